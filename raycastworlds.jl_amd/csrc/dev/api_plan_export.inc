// Development build only (-DRCW_DEV_SWITCHES): the top view's rule and its table of thresholds WITHOUT a device — what
// tests/test_top_view_plan.py runs on the CPU.  A fragment of rcw_api.hip, included behind plan_top_view (inside the anonymous namespace: the
// two exports leave it and come back).
}  // namespace
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
    const int form = !d.top_view ? RCW_TOP_VIEW_NONE : d.top_split ? RCW_TOP_VIEW_TWO_KERNELS : d.top_lds ? RCW_TOP_VIEW_ONE_KERNEL : RCW_TOP_VIEW_IN_PLACE;
    const int alone = !d.top_view ? RCW_TOP_VIEW_NONE : (d.top_split && d.top_alone_split) ? RCW_TOP_VIEW_TWO_KERNELS : d.top_lds ? RCW_TOP_VIEW_ONE_KERNEL : RCW_TOP_VIEW_IN_PLACE;
    const int32_t v[16] = {form, alone, d.top_lds, d.top_split, d.top_flat, d.top_unit_px, d.top_fused, d.top_draw_first, d.top_parts, d.top_runs,
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
}  // extern "C"
namespace {
