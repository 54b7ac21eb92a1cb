// Development build only (-DRCW_DEV_SWITCHES): the top view's rule and its table of thresholds WITHOUT a device — what
// tests/test_top_view_plan.py runs on the CPU.  The tail of rcw_rules.hip, at file scope.
extern "C" {
// out[16]: form in a step (RCW_TOP_VIEW_*), form of rcw_update_top_view alone, then top_lds, top_split, top_flat, top_unit_px, top_fused,
// top_draw_first, top_parts, top_runs, top_draw_block, top_draw_block_alone, top_alone_split, top_grid, top_store_grid, return code
__attribute__((visibility("default"))) int rcw_dev_plan_top_view(const rcw_config* cfg, int32_t batch, int32_t cus, int32_t lds_per_cu, int32_t waves_per_cu,
                                                                int32_t want_form, int32_t want_runs, int32_t* out)
{
    if (!cfg || !out || batch < 1 || cus < 1) return RCW_ERR_INVALID_ARGUMENT;
    RcwPlan d{};
    set_geometry(d, cfg, batch);
    d.fill_grid = cus;
    d.top_view = cfg->render_top_view ? reinterpret_cast<uint32_t*>(16) : nullptr;      // (a marker: the rule only asks whether the handle renders one)
    const RcwHw hw{cus, lds_per_cu, waves_per_cu};
    const int rc = top_view_rule(d, cfg, (size_t)batch, hw, want_form, want_runs, /*lenient=*/want_form == 0);
    const int32_t v[16] = {top_form_in_step(d), top_form_alone(d), d.top_lds, d.top_split, d.top_flat, d.top_unit_px, d.top_fused, d.top_draw_first, d.top_parts, d.top_runs,
                           d.top_draw_block, d.top_draw_block_alone, d.top_alone_split, d.top_grid, d.top_store_grid, rc};
    std::memcpy(out, v, sizeof v);
    return rc;
}
// the table as text, a rule a line: name <tab> value <tab> unit <tab> evidence; returns the bytes written (without the terminator), -1 if buf is too small
__attribute__((visibility("default"))) int rcw_dev_top_view_rules(char* buf, int32_t cap)
{
    if (!buf || cap < 1) return -1;
    int n = 0;
    for (int k = 0; k < kTopRuleCount; ++k) {
        const int w = std::snprintf(buf + n, (size_t)(cap - n), "%s\t%.17g\t%s\t%s\n", kTopRules[k].name, kTopRules[k].value, kTopRules[k].unit, kTopRules[k].evidence);
        if (w < 0 || n + w >= cap) return -1;
        n += w;
    }
    return n;
}
// the step's rule without a device: 1 where a handle of this configuration and batch takes the one-launch step by itself (rcw_step_form after
// rcw_create), 0 where it keeps the two launches (geometry or batch), as step_one_launch_pays and rcw_step_spec_eligible decide
__attribute__((visibility("default"))) int rcw_dev_step_rule(const rcw_config* cfg, int32_t batch, int32_t cus)
{
    if (!cfg || batch < 1 || cus < 1) return RCW_ERR_INVALID_ARGUMENT;
    RcwPlan d{};
    set_geometry(d, cfg, batch);
    d.fill_grid = cus;
    d.top_view = cfg->render_top_view ? reinterpret_cast<uint32_t*>(16) : nullptr;
    return rcw_step_spec_eligible(d) && step_one_launch_pays(d) ? 1 : 0;
}
// A StepFacts driven through a list of events without a device (tests/test_step_state.py).  `eligible`, `pays`: what rcw_step_spec_eligible and
// step_one_launch_pays would say of the handle.  events [n][3] = kind, a, b; out [n][12] = the nine facts behind each event (StepFacts::read),
// then, for a camera step, the path it took (StepFacts::Path; else -1) and the `keep` it passes, then 1 where the event was refused.
//   0  plan_step_form(want = a), the learner view with RCW_VIEW_ONLY: b
//   1  launch_step_camera; a: bit 0 actions, bit 1 a mask, bit 2 the stream is capturing, bit 3 the first launch fails, bit 4 the priming path's fill fails
//   2  a RCW_VIEW_ONLY step (launch_step); a: bit 1 a mask             3  rcw_bind_obs
//   4  rcw_reset in front of its render; a: bit 0 a mask, bit 1 a seed that is not the handle's, bit 2 cfg.auto_reset
//   5  rcw_cast_rays, or ensure_columns in front of a reader           6  rcw_columns_device_ptr / a learner view switched on
//   7  rcw_update_camera_view                                         8  rcw_set_time_limit
//   9  rcw_snapshot_restore* behind its gather, in front of its render (an event 1 without an action, with the call's mask)
__attribute__((visibility("default"))) int rcw_dev_step_facts(int32_t eligible, int32_t pays, int32_t store_all, const int32_t* events, int32_t n, int32_t* out)
{
    if (!events || !out || n < 0) return RCW_ERR_INVALID_ARGUMENT;
    StepFacts f;
    f.set_store_all(store_all != 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t kind = events[3 * i], a = events[3 * i + 1], b = events[3 * i + 2];
        const bool masked = (a & 2) != 0;
        int32_t* const o = out + 12 * (size_t)i;
        o[9] = -1; o[10] = 0; o[11] = 0;
        if (kind == 0) {
            const StepFacts::Plan p = f.plan(a, b != 0, eligible != 0, pays != 0);
            if (p.refused) o[11] = 1; else f.take(p);
        } else if (kind == 1) {
            const StepFacts::Camera c = f.camera_step((a & 1) != 0, masked, [a] { return (a & 4) != 0; });
            o[9] = c.path; o[10] = c.keep;
            if (c.path == StepFacts::kOneLaunch && !(a & 8)) f.one_launch_queued();
            if (c.path == StepFacts::kPrime && !(a & 8)) { f.prime_cast_queued(masked); if (!(a & 16)) f.prime_fill_queued(c, masked); }
        }
        else if (kind == 2) { f.obs_unknown(); f.columns_cast(masked); }
        else if (kind == 3) f.obs_unknown();
        else if (kind == 4) f.reset((a & 1) != 0, (a & 2) != 0, (a & 4) != 0);
        else if (kind == 5) f.columns_cast();
        else if (kind == 6) { f.columns_wanted(); f.columns_cast(); }
        else if (kind == 7) { f.obs_unknown(); f.columns_cast(); f.camera_repainted(); }
        else if (kind == 8) f.time_limit_set();
        else if (kind == 9) f.restored();
        else return RCW_ERR_INVALID_ARGUMENT;
        f.read(o);
    }
    return n;
}
// rcw_set_walls' host validation without a handle (tests/test_walls_spec.py): the return code of validate_walls, its reason in msg
__attribute__((visibility("default"))) int rcw_dev_validate_walls(int32_t H, int32_t W, int32_t batch, const uint8_t* walls, int32_t layouts,
                                                                 const int32_t* index, const uint8_t* mask, char* msg, int32_t cap)
{
    if (!msg || cap < 1 || H < 3 || W < 3 || batch < 1) return RCW_ERR_INVALID_ARGUMENT;
    msg[0] = 0;
    return validate_walls(H, W, batch, walls, layouts, index, mask, msg, (size_t)cap);
}
// The state archive's record without a device (tests/test_snapshot_spec.py).  shape: the 23 Int32 of SnapshotShape in its order — H, W, nd, N,
// Hc, real64, reward_type | goal, seen, stats | view_fmt, view_layout, view_C, view_h, view_w, view_frames | local_source, local_size,
// local_cells | source_kind | layouts, levels, first_level.  names: the segments' names, a line each; bytes [n]; returns n, -1: names too small.
static_assert(sizeof(SnapshotShape) == (kSnapshotShapeWords + 5) * sizeof(int32_t) && kSnapshotVisitWords == kSnapshotShapeWords + 4, "SnapshotShape travels as its first 23 Int32: the guide and the frontier, which are no part of a record, the visit map (rcw_dev_visit_plan takes 27) and the start rule stay off");
__attribute__((visibility("default"))) int rcw_dev_snapshot_plan(const int32_t* shape, char* names, int32_t cap, uint32_t* bytes, uint64_t* row_bytes, uint64_t* key)
{
    if (!shape || !names || cap < 1 || !bytes || !row_bytes || !key) return RCW_ERR_INVALID_ARGUMENT;
    SnapshotShape sh;
    std::memcpy(&sh, shape, kSnapshotShapeWords * sizeof(int32_t));
    SnapshotPlan plan;
    plan_snapshot(sh, &plan);
    int n = 0;
    for (int k = 0; k < plan.n; ++k) {
        const int w = std::snprintf(names + n, (size_t)(cap - n), "%s\n", plan.seg[k].name);
        if (w < 0 || n + w >= cap) return -1;
        n += w;
        bytes[k] = plan.seg[k].bytes;
    }
    *row_bytes = plan.row_bytes; *key = plan.key;
    return plan.n;
}
// The per-agent arrays of one feature (AgentFeature: 0 core state, 1 goal distance, 2 seen map, 3 learner view, 4 local map, 5 layout source,
// 6 episode statistics, 7 the guide, 8 the frontier, 9 the visit map, 10 the start rule — all four off in every shape that travels here) of that shape, and their carve for `batch` agents as ONE buffer behind the feature's head (tests/
// test_agent_arrays_spec.py): names a line each; ids, bytes (per agent), archived, offsets [n]; returns n (0: the feature is off), -1: names
// too small.
__attribute__((visibility("default"))) int rcw_dev_agent_arrays(const int32_t* shape, int32_t feature, int32_t batch, char* names, int32_t cap, int32_t* ids,
                                                               uint32_t* bytes, uint8_t* archived, uint64_t* offsets, uint64_t* head, uint64_t* total)
{
    if (!shape || feature < 0 || feature >= kFeatCount || batch < 1 || !names || cap < 1 || !ids || !bytes || !archived || !offsets || !head || !total) return RCW_ERR_INVALID_ARGUMENT;
    SnapshotShape sh;
    std::memcpy(&sh, shape, kSnapshotShapeWords * sizeof(int32_t));
    AgentArrays a;
    agent_arrays(sh, feature, &a);
    const AgentCarve c = carve_agent_arrays(a.head, a.part, a.n, (uint64_t)batch);
    int n = 0;
    names[0] = 0;
    for (int k = 0; k < a.n; ++k) {
        const int w = std::snprintf(names + n, (size_t)(cap - n), "%s\n", a.part[k].name);
        if (w < 0 || n + w >= cap) return -1;
        n += w;
        ids[k] = a.part[k].id; bytes[k] = a.part[k].bytes; archived[k] = a.part[k].archived; offsets[k] = c.off[k];
    }
    *head = a.head; *total = c.total;
    return a.n;
}
// The guide's promise for a configuration without a device (tests/test_guide_spec.py): what rcw_guide_info reports as `promised`
__attribute__((visibility("default"))) int rcw_dev_guide_promised(const rcw_config* cfg)
{
    return cfg ? guide_promised(*cfg) : RCW_ERR_INVALID_ARGUMENT;
}
// The frontier's arrays and the record of a shape WITH the frontier on (tests/test_frontier_spec.py; `frontier` does not travel in the 23
// words): names a line each, bytes (per agent) and archived [n] of kFeatFrontier's parts; the plan's segment count, row bytes and key — to be
// held to rcw_dev_snapshot_plan's of the same 23 words.  Returns n, -1: names too small.
__attribute__((visibility("default"))) int rcw_dev_frontier_plan(const int32_t* shape, char* names, int32_t cap, uint32_t* bytes, uint8_t* archived,
                                                                 int32_t* segments, uint64_t* row_bytes, uint64_t* key)
{
    if (!shape || !names || cap < 1 || !bytes || !archived || !segments || !row_bytes || !key) return RCW_ERR_INVALID_ARGUMENT;
    SnapshotShape sh;
    std::memcpy(&sh, shape, kSnapshotShapeWords * sizeof(int32_t));
    sh.frontier = 1;
    AgentArrays a;
    agent_arrays(sh, kFeatFrontier, &a);
    int n = 0;
    for (int k = 0; k < a.n; ++k) {
        const int m = std::snprintf(names + n, (size_t)(cap - n), "%s\n", a.part[k].name);
        if (m < 0 || m >= cap - n) return -1;
        n += m;
        bytes[k] = a.part[k].bytes; archived[k] = a.part[k].archived ? 1 : 0;
    }
    SnapshotPlan plan;
    plan_snapshot(sh, &plan);
    *segments = plan.n; *row_bytes = plan.row_bytes; *key = plan.key;
    return a.n;
}
// The visit map's arrays, table and record from the WHOLE shape (tests/test_visit_map_spec.py): `shape` holds all `words` Int32 of
// SnapshotShape in its order but the last, `start`, which stays off — the 23 above, guide, frontier, visit_sectors, visit_flags.  names a line each, bytes (per agent), archived and
// the carve's offsets for `batch` agents [n] of kFeatVisits' parts, the head (the table's bytes) and the carve's total; the table's rows
// and first level (plan_visit_table_rows; zeros without RCW_VISIT_TABLE); the plan's segment count, row bytes and key.  Returns n (0: off),
// -1: names too small.
__attribute__((visibility("default"))) int rcw_dev_visit_plan(const int32_t* shape, int32_t words, int32_t batch, char* names, int32_t cap, uint32_t* bytes,
                                                              uint8_t* archived, uint64_t* offsets, uint64_t* head, uint64_t* total, int32_t* rows,
                                                              int32_t* first_level, int32_t* segments, uint64_t* row_bytes, uint64_t* key)
{
    if (!shape || words != kSnapshotVisitWords || batch < 1 || !names || cap < 1 || !bytes || !archived || !offsets || !head ||
        !total || !rows || !first_level || !segments || !row_bytes || !key) return RCW_ERR_INVALID_ARGUMENT;
    SnapshotShape sh;
    std::memcpy(&sh, shape, kSnapshotVisitWords * sizeof(int32_t));
    if (sh.H < 1 || sh.W < 1 || sh.visit_sectors < 0 || sh.visit_sectors > RCW_VISIT_MAX_SECTORS || (int64_t)sh.H * sh.W > INT32_MAX / (2 * RCW_VISIT_MAX_SECTORS)) return RCW_ERR_INVALID_ARGUMENT;
    AgentArrays a;
    agent_arrays(sh, kFeatVisits, &a);
    const AgentCarve c = carve_agent_arrays(a.head, a.part, a.n, (uint64_t)batch);
    int n = 0;
    names[0] = 0;
    for (int k = 0; k < a.n; ++k) {
        const int m = std::snprintf(names + n, (size_t)(cap - n), "%s\n", a.part[k].name);
        if (m < 0 || m >= cap - n) return -1;
        n += m;
        bytes[k] = a.part[k].bytes; archived[k] = a.part[k].archived ? 1 : 0; offsets[k] = c.off[k];
    }
    *head = a.head; *total = c.total;
    *rows = 0; *first_level = 0;
    if (sh.visit_sectors && (sh.visit_flags & RCW_VISIT_TABLE)) plan_visit_table_rows(sh, rows, first_level);
    SnapshotPlan plan;
    plan_snapshot(sh, &plan);
    *segments = plan.n; *row_bytes = plan.row_bytes; *key = plan.key;
    return a.n;
}
// rcw_snapshot_rows_load's check of one exported row of that shape: validate_snapshot_row's return code, its reason in msg
__attribute__((visibility("default"))) int rcw_dev_snapshot_validate_row(const int32_t* shape, const uint8_t* row, char* msg, int32_t cap)
{
    if (!shape || !row || !msg || cap < 1) return RCW_ERR_INVALID_ARGUMENT;
    SnapshotShape sh;
    std::memcpy(&sh, shape, kSnapshotShapeWords * sizeof(int32_t));
    if (sh.H < 3 || sh.W < 3 || sh.nd < 1) return RCW_ERR_INVALID_ARGUMENT;
    SnapshotPlan plan;
    plan_snapshot(sh, &plan);
    msg[0] = 0;
    return validate_snapshot_row(sh, plan, row, msg, (size_t)cap);
}
}  // extern "C"
