// What a step, a reset or a re-render of a handle launches, and the resources those launches need: the launch sequences of a step and of
// the two-kernel top view, the buffers of the forms a handle takes, and the handle's one teardown.
#include "rcw_handle.h"

#include <hip/hip_runtime.h>

#include <utility>

namespace {

// The four profiling events of ONE step, or none (profiling off, slots used up): mark(k) records event k on a stream, done() the last one on
// the handle's stream — and, recorded, counts the step: one that failed on the way is not counted.
class Bracket {
    rcw_handle::Profile* p_;
public:
    explicit Bracket(rcw_handle::Profile* p = nullptr) : p_(p && p->on && p->count < p->kSlots ? p : nullptr) {}
    hipError_t mark(int k, hipStream_t s) const { return p_ ? hipEventRecord(p_->ev[4 * p_->count + k].get(), s) : hipSuccess; }
    hipError_t done(hipStream_t s) const { const hipError_t e = mark(3, s); if (p_ && e == hipSuccess) p_->count++; return e; }
};

// update_top_view!(env) SR:446-483.  Two-kernel form: the draw kernel (VALU/LDS work, planes -> HBM) and the
// moving-window store kernel.  `between` (the camera fill, inside a step) is launched on the handle's stream while
// the draw kernel runs on the side stream: fork after what is already queued (the cast kernel), join before the store.
// The stand-alone call (`beside` = false) has no camera fill to run beside and takes the one-kernel form.
template <typename Between>
hipError_t launch_top_view_ordered(rcw_handle* h, const uint8_t* mask_dev, bool beside, Between between, const Bracket& prof);
template <typename Between>
hipError_t launch_top_view(rcw_handle* h, const uint8_t* mask_dev, bool beside, Between between, const Bracket& prof = Bracket())   // between(stream): the caller's camera fill
{
    const RcwPlan& d = h->dev;
    hipError_t e;
    if (!d.top_split || (!beside && !d.top_alone_split)) {   // (nothing to hide the draw kernel behind: the one-kernel form is the faster one)
        if ((e = rcw_launch_top_view(d, mask_dev, h->stream)) != hipSuccess) return e;
        return between(h->stream);
    }
    if (d.top_parts > 1) {                                   // (see rcw_handle::top_plane_dirty; every order below forks from the handle's stream behind this)
        if (h->top_plane_dirty && (e = hipMemsetAsync(h->d_top_plane.get(), 0, rcw_top_plane_bytes(d), h->stream)) != hipSuccess) return e;
        h->top_plane_dirty = true;
        struct Clean { rcw_handle* h; hipError_t* e; ~Clean() { if (*e == hipSuccess) h->top_plane_dirty = false; } };
        hipError_t result = hipErrorUnknown;
        Clean clean{h, &result};
        result = launch_top_view_ordered(h, mask_dev, beside, between, prof);
        return result;
    }
    return launch_top_view_ordered(h, mask_dev, beside, between, prof);
}

// (the launch orders of the two-kernel form; launch_top_view above decides whether it is taken)
template <typename Between>
hipError_t launch_top_view_ordered(rcw_handle* h, const uint8_t* mask_dev, bool beside, Between between, const Bracket& prof)
{
    const RcwPlan& d = h->dev;
    hipError_t e;
    if (!beside) {                                           // stand-alone, two kernels back to back on the handle's stream
        if ((e = rcw_launch_top_draw(d, mask_dev, 0, d.B, h->stream, d.top_draw_block_alone)) != hipSuccess) return e;
        if ((e = rcw_launch_top_store(d, mask_dev, 0, d.B, h->stream)) != hipSuccess) return e;
        return between(h->stream);
    }
    if (d.top_fused) {
        // the camera fill and the drawing in ONE launch (rcw_fill256_draw_kernel), then the store: three launches on one
        // stream, no fork / join.  `between` — the camera fill of the caller — is replaced by that launch; its profiling
        // event (behind the fill, in front of the store kernel) is recorded here.
        if ((e = rcw_launch_fill256_draw(d, mask_dev, h->stream)) != hipSuccess) return e;
        if ((e = prof.mark(2, h->stream)) != hipSuccess) return e;
        return rcw_launch_top_store(d, mask_dev, 0, d.B, h->stream);
    }
    if (d.top_draw_first && d.top_runs <= 1) {
        // The DRAWING stays on the handle's stream, right behind the cast kernel, and the store kernel right behind the drawing; the camera
        // fill — which nothing of the top view depends on — goes to the side stream.  Measured with rocprofv3's kernel trace (tools/
        // step_timeline.sh): a kernel behind an event of the other stream starts ~13 us later than one behind a kernel of its own stream (19
        // against 6 us after the cast kernel's end), and the store kernel behind the join another 13 us after the drawing's end — with the
        // drawing on the side stream both lie on the step's critical path wherever the drawing outlasts the fill.  This way the late start
        // is the fill's, which has the drawing's whole time to spare, and the join at the end waits for a fill that ended long ago.
        if ((e = hipEventRecord(h->ev_top_fork.get(), h->stream)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(h->top_stream.get(), h->ev_top_fork.get(), 0)) != hipSuccess) return e;
        e = between(h->top_stream.get());                              // (its profiling event is recorded on that stream too)
        const hipError_t rec = hipEventRecord(h->ev_top_join[0].get(), h->top_stream.get());
        if (e == hipSuccess) e = rcw_launch_top_draw(d, mask_dev, 0, d.B, h->stream);
        if (e == hipSuccess) e = rcw_launch_top_store(d, mask_dev, 0, d.B, h->stream);
        if (rec == hipSuccess) { const hipError_t w = hipStreamWaitEvent(h->stream, h->ev_top_join[0].get(), 0); if (e == hipSuccess) e = w; }
        return e == hipSuccess ? rec : e;
    }
    if ((e = hipEventRecord(h->ev_top_fork.get(), h->stream)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(h->top_stream.get(), h->ev_top_fork.get(), 0)) != hipSuccess) return e;
    // The batch goes in d.top_runs runs of agents (one, unless the batch is several GiB of top view AND the drawing is
    // long against the camera fill): the side stream draws run after run without waiting for anything, the handle's
    // stream stores run r as soon as it is drawn — so what of the drawing does not fit beside the camera fill runs beside
    // the (HBM-bound) storing of earlier runs.
    // From here on the side stream may hold work: whatever fails, the handle's stream joins it again (every recorded
    // event is waited for), so that nothing runs on the side stream that the handle's stream does not wait for — a
    // later rcw_set_stream synchronises the handle's stream only, and a capture must end joined.
    const int runs = d.top_runs > 1 ? d.top_runs : 1;
    int recorded = 0;
    for (int r = 0; r < runs && e == hipSuccess; ++r) {
        const int first = (int)((long long)d.B * r / runs), count = (int)((long long)d.B * (r + 1) / runs) - first;
        e = rcw_launch_top_draw(d, mask_dev, first, count, h->top_stream.get());
        const hipError_t rec = hipEventRecord(h->ev_top_join[r].get(), h->top_stream.get());    // (also after a failed launch: earlier runs' draws are queued)
        if (rec == hipSuccess) recorded = r + 1;
        if (e == hipSuccess) e = rec;
    }
    if (e == hipSuccess) e = between(h->stream);
    for (int r = 0; r < recorded; ++r) {
        const int first = (int)((long long)d.B * r / runs), count = (int)((long long)d.B * (r + 1) / runs) - first;
        const hipError_t w = hipStreamWaitEvent(h->stream, h->ev_top_join[r].get(), 0);
        if (e == hipSuccess) e = w;
        if (e == hipSuccess) e = rcw_launch_top_store(d, mask_dev, first, count, h->stream);
    }
    return e;
}

// Every stream that may hold work of the handle — the side stream, its own, the caller's current one — is waited for; the first failure comes back.
hipError_t wait_all_streams(rcw_handle* h)
{
    hipError_t e = hipSuccess;
    for (hipStream_t s : {h->top_stream.get(), h->own_stream.get(), h->stream != h->own_stream.get() ? h->stream : nullptr})
        if (s) { const hipError_t r = hipStreamSynchronize(s); if (e == hipSuccess) e = r; }
    return e;
}

}  // namespace

// update_top_view! with no camera fill to run beside: rcw_update_top_view, and a RCW_VIEW_ONLY step between its cast and its view kernel
hipError_t launch_top_view_alone(rcw_handle* h, const uint8_t* mask_dev)
{
    return launch_top_view(h, mask_dev, false, [](hipStream_t) { return hipSuccess; });
}

// the camera fill of the handle's own descriptors into dev.obs (the unmasked agents' frames only)
hipError_t paint_camera(rcw_handle* h, const uint8_t* mask_dev, hipStream_t stream)
{
    return rcw_launch_fill(h->dev, h->dev.col_h, h->dev.col_c, h->dev.obs, (long long)h->dev.B * h->dev.N, mask_dev, stream);
}

// ... or, behind the layout source's kernel (sparse: the mask is the source's, nearly always empty), a workgroup an agent instead of the window's sweep
hipError_t paint_camera(rcw_handle* h, const uint8_t* mask_dev, hipStream_t stream, bool sparse)
{
    return sparse ? rcw_launch_wall_bank_paint(h->dev, mask_dev, stream) : paint_camera(h, mask_dev, stream);
}

// A step's camera view is one of three sequences of launches (launch_step_camera chooses: StepFacts::camera_step).  With profiling on, HIP
// events bracket each kernel (Bracket): start (launch_step_camera's) | after cast | after the top view or the fill | end.
namespace {

// act!(env, a) SR:333-340 in ONE launch: the fill workgroups write the frames the actions select among the successors the last casting
// launch left in the current slot buffer; the casting workgroups commit the actions and cast the new states' successors into the other one
hipError_t launch_step_one(rcw_handle* h, const uint8_t* actions_dev, bool keep, const Bracket& prof)
{
    rcw_handle::Step& st = h->step;
    hipError_t e;
    if ((e = prof.mark(1, h->stream)) != hipSuccess || (e = prof.mark(2, h->stream)) != hipSuccess) return e;
    if ((e = rcw_launch_step_spec(h->dev, actions_dev, nullptr, st.slot[st.cur()].get<uint16_t>(), st.slot[st.cur() ^ 1].get<uint16_t>(), true, st.cols_live(), keep, h->stream)) != hipSuccess) return e;
    st.one_launch_queued();
    return prof.done(h->stream);
}

// reset! / set_state (no action, maybe a mask) or a first step of the one-launch form: the casting workgroups alone — dynamics if any, the
// current frame's descriptors, and the (masked) agents' slots in place —, then the camera fill as a launch of its own
hipError_t launch_step_prime(rcw_handle* h, const uint8_t* actions_dev, const uint8_t* mask_dev, const StepFacts::Camera& c, const Bracket& prof, bool sparse)
{
    rcw_handle::Step& st = h->step;
    hipError_t e;
    if ((e = rcw_launch_step_spec(h->dev, actions_dev, mask_dev, nullptr, st.slot[st.cur()].get<uint16_t>(), false, true, false, h->stream)) != hipSuccess) return e;
    st.prime_cast_queued(mask_dev != nullptr);
    if ((e = prof.mark(1, h->stream)) != hipSuccess || (e = prof.mark(2, h->stream)) != hipSuccess) return e;
    if ((e = paint_camera(h, mask_dev, h->stream, sparse)) != hipSuccess) return e;
    st.prime_fill_queued(c, mask_dev != nullptr);
    return prof.done(h->stream);
}

// cast kernel + fill kernel, back to back on the handle's stream (+ the top view when the handle renders it: before the fill with the
// one-kernel form, around it with the two-kernel form, whose event 2 is behind the fill)
hipError_t launch_step_two(rcw_handle* h, const uint8_t* actions_dev, const uint8_t* mask_dev, const Bracket& prof, bool sparse)
{
    const RcwPlan& d = h->dev;
    hipError_t e;
    if ((e = rcw_launch_cast(d, actions_dev, mask_dev, h->stream)) != hipSuccess) return e;
    if ((e = prof.mark(1, h->stream)) != hipSuccess) return e;
    auto fill = [&](hipStream_t fs) -> hipError_t {            // (fs: the handle's stream, or its side stream: launch_top_view)
        hipError_t f;
        if (!d.top_split && (f = prof.mark(2, fs)) != hipSuccess) return f;
        if ((f = paint_camera(h, mask_dev, fs, sparse && !d.top_view)) != hipSuccess) return f;   // (with a top view the fill may be the launch that draws)
        return d.top_split ? prof.mark(2, fs) : hipSuccess;
    };
    if ((e = d.top_view ? launch_top_view(h, mask_dev, true, fill, prof) : fill(h->stream)) != hipSuccess) return e;   // SR:337
    return prof.done(h->stream);
}

// (bank = true: the layout source's re-render of the agents it restarted — behind the step proper, outside its bracket, the mask sparse)
hipError_t launch_step_camera(rcw_handle* h, const uint8_t* actions_dev, const uint8_t* mask_dev, bool bank = false)
{
    const StepFacts::Camera c = h->step.camera_step(actions_dev != nullptr, mask_dev != nullptr, [h] {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        return hipStreamIsCapturing(h->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    });
    const Bracket prof(bank ? nullptr : &h->prof);
    const hipError_t e = prof.mark(0, h->stream);
    if (e != hipSuccess) return e;
    if (c.path == StepFacts::kOneLaunch) return launch_step_one(h, actions_dev, c.keep, prof);
    if (c.path == StepFacts::kPrime) return launch_step_prime(h, actions_dev, mask_dev, c, prof, bank);
    return launch_step_two(h, actions_dev, mask_dev, prof, bank);
}

}  // namespace

// the learner view of the handle's current descriptors (the unmasked agents' only), on the handle's stream; with a frame stack the view
// kernel's frame is the staging batch and the push kernel follows it
hipError_t launch_view(rcw_handle* h, const uint8_t* mask_dev, StackOp op)
{
    const rcw_handle::LearnerView& lv = h->learner;
    if (lv.set.frames < 2 || op == kStackKeep)
        return rcw_launch_view(h->dev, lv.view, h->dev.col_h, h->dev.col_c, h->B, mask_dev, lv.frame.get<uint8_t>(), h->stream);
    return rcw_launch_view_stack(h->dev, lv.view, h->dev.col_h, h->dev.col_c, h->B, lv.set.frames, mask_dev, lv.frame.get<uint8_t>(),
                                 lv.stack.get<uint8_t>(), h->dev.episode, lv.last_episode.get<uint32_t>(), op != kStackPush, h->stream);
}

// A step, reset! or set_state's render: the camera view (launch_step_camera), then the learner view where the handle has one.  With
// RCW_VIEW_ONLY the cast kernel is followed by the view kernel alone (the top view, if any, in its stand-alone form between them);
// profiling events: start | after cast | after the top view | after the view kernel.
// Last of all, and OUTSIDE the profiling bracket (cast_ms + top_view_ms + fill_ms is what it was), the goal distance where the handle has
// enabled it: behind a step (the episode counter decides who floods) or a reset / set_state / set_walls (the mask decides).
hipError_t launch_goal_distance(rcw_handle* h, const uint8_t* mask_dev, StackOp op)
{
    if (!h->goal.on() || op == kStackKeep || op == kStackRefillSameWorld) return hipSuccess;
    return rcw_launch_goal_distance(h->dev, h->B, mask_dev, op == kStackRefill, h->goal.field.get<uint16_t>(), h->goal.words,
                                    h->goal.last_episode.get<uint32_t>(), h->stream);
}

// ... and behind it, on the same terms, the seen map: behind a step the counter decides who is cleared, behind a refill the mask
hipError_t launch_seen_map(rcw_handle* h, const uint8_t* mask_dev, StackOp op)
{
    if (!h->seen.on() || op == kStackKeep || op == kStackRefillSameWorld) return hipSuccess;
    return rcw_launch_seen_map(h->dev, h->B, mask_dev, op == kStackRefill, h->seen.map, h->seen.bits, h->seen.words, h->seen.last_episode, h->stream);
}

// ... and directly behind the seen map, the frontier, which floods over it.  Behind a step the agents whose map changed or whose episode began
// flood (the kernel reads the seen map's newly_seen word and its own recorded counter), behind a refill those of the mask; the action words
// are a pure function of (field, position, heading, direction table) and follow for every agent, through the guide's kernel on THIS field —
// also behind a new direction table (kStackRefillSameWorld), where nothing floods.  launch_snapshot asks for the masked refill behind a
// restore's render.  A re-render of the very same frames (kStackKeep) launches nothing.
hipError_t launch_frontier(rcw_handle* h, const uint8_t* mask_dev, StackOp op)
{
    const rcw_handle::Frontier& fr = h->frontier;
    if (!fr.on() || !h->seen.on() || op == kStackKeep) return hipSuccess;
    if (op != kStackRefillSameWorld) {
        const hipError_t e = rcw_launch_frontier(h->dev, h->B, mask_dev, op == kStackRefill, h->seen.map, h->seen.words.newly_seen, fr.field, fr.words,
                                                 fr.last_episode, h->stream);
        if (e != hipSuccess) return e;
    }
    return rcw_launch_guide(h->dev, h->B, fr.field, fr.advice, h->stream);
}

// ... and the visit map, behind the frontier and in front of the local map: pose, episode counter and layout word are final there (the
// layout source's kernel and its re-render have run).  A step runs the step rule (the counter decides who begins), a refill the mask rule;
// a re-render of the same world (a new direction table, a change of the step's form, a restore's render) launches nothing: a restore puts
// the record back and counts nothing.
hipError_t launch_visit_map(rcw_handle* h, const uint8_t* mask_dev, StackOp op)
{
    if (!h->visits.on() || op == kStackKeep || op == kStackRefillSameWorld) return hipSuccess;
    return rcw_launch_visit_map(h->dev, h->B, h->visits.dev, h->source.live() ? h->source.dev.agents.layout : nullptr, mask_dev, op == kStackRefill, h->stream);
}

// ... and last, behind the seen map it may read, the local map: a pure function of the state, so every agent's image at every render but
// the one that re-renders the very same frames
hipError_t launch_local_map(rcw_handle* h, StackOp op)
{
    const rcw_handle::LocalMap& lm = h->local;
    if (!lm.on() || op == kStackKeep) return hipSuccess;
    return rcw_launch_local_map(h->dev, h->B, lm.source == RCW_LOCAL_SEEN ? h->seen.map : nullptr, lm.off, lm.size, lm.img, h->stream);
}

// ... and episode statistics, behind the goal distance (whose start_distance a close reads) and the layout source (whose layout it reads),
// both as they are NOW — NULL where the handle has none.  A step runs the step rule, a refill the mask rule; a re-render of the same world
// (a new direction table, a change of the step's form) launches nothing.
hipError_t launch_episode_stats(rcw_handle* h, const uint8_t* mask_dev, StackOp op)
{
    if (!h->stats.on() || op == kStackKeep || op == kStackRefillSameWorld) return hipSuccess;
    return rcw_launch_episode_stats(h->dev, h->dev.limit, h->stats.dev, h->source.live() ? h->source.dev.agents.layout : nullptr,
                                    h->goal.on() ? h->goal.words.start_distance : nullptr, mask_dev, op == kStackRefill, h->stream);
}

// ... and the guide, directly behind the goal distance whose field it reads.  A pure function of (field, position, heading, direction table), for every
// agent: it also runs where the goal distance does not — behind a new direction table (kStackRefillSameWorld) —, and launch_snapshot asks
// for it behind a restore's render.  A re-render of the very same frames (kStackKeep) changes none of the four and launches nothing.
hipError_t launch_guide(rcw_handle* h, StackOp op)
{
    if (!h->guide.on() || !h->goal.on() || op == kStackKeep) return hipSuccess;
    return rcw_launch_guide(h->dev, h->B, h->goal.field.get<uint16_t>(), h->guide.words, h->stream);
}

// The layout source (rcw_handle::LayoutSource), behind the core launches of a call that can move an episode counter: its kernel gives every
// agent that began an episode a layout and a fresh state against it, and leaves in the source's own mask who that was.  force: every agent
// (the call that installs the source).  Behind rcw_reset the caller's re-render covers exactly those agents; behind a step, launch_step
// re-renders them.  A handle without a source launches nothing.
hipError_t launch_layout_source(rcw_handle* h, bool force)
{
    return rcw_launch_layout_source(h->dev, h->source.dev, force, h->stream);
}

// The start rule (rcw_handle::StartRule), directly behind launch_layout_source wherever that is called: its kernel moves every agent that
// began an episode in the call (force: every agent) to a tile of the band and leaves in its own mask who that was — a superset of the
// source's: both key on the counter moving in the same call.  A handle without the rule launches nothing.
hipError_t launch_start_distance(rcw_handle* h, bool force)
{
    if (!h->start.on()) return hipSuccess;
    return rcw_launch_start_distance(h->dev, h->start.dev, (uint32_t)h->start.lo, (uint32_t)h->start.hi, force, h->stream);
}

// A step of a handle with a layout source: the step proper, the source's kernel, the camera view of the agents it restarted once more through
// the masked path (valid in both step forms: a masked prime behind a one-launch step is what rcw_set_walls(mask) queues) — all OUTSIDE
// rcw_profile's bracket —, and then every feature ONCE: they key on the episode counter and find the restarted agents stale against the
// final world.  A handle with the start rule does the same, source or not: the rule's kernel follows the source's, and the ONE re-render
// takes the rule's mask, which covers the source's.  A handle with neither launches what it launched before.
hipError_t launch_step(rcw_handle* h, const uint8_t* actions_dev, const uint8_t* mask_dev, StackOp op)
{
    const uint8_t* const restarted = h->start.on() ? h->start.dev.mask : h->source.dev.agents.mask;   // (whom the kernels restarted; NULL with neither)
    const bool restarts = (h->source.live() || h->start.on()) && actions_dev != nullptr;
    if (!h->learner.only()) {
        hipError_t e = launch_step_camera(h, actions_dev, mask_dev);
        if (e == hipSuccess && restarts) e = launch_layout_source(h, false);
        if (e == hipSuccess && restarts) e = launch_start_distance(h, false);
        if (e == hipSuccess && restarts) e = launch_step_camera(h, nullptr, restarted, true);
        if (e == hipSuccess && h->learner.on()) e = launch_view(h, mask_dev, op);
        if (e == hipSuccess) e = launch_goal_distance(h, mask_dev, op);
        if (e == hipSuccess) e = launch_guide(h, op);
        if (e == hipSuccess) e = launch_seen_map(h, mask_dev, op);
        if (e == hipSuccess) e = launch_frontier(h, mask_dev, op);
        if (e == hipSuccess) e = launch_visit_map(h, mask_dev, op);
        if (e == hipSuccess) e = launch_local_map(h, op);
        return e == hipSuccess ? launch_episode_stats(h, mask_dev, op) : e;
    }
    h->step.obs_unknown();                                        // (the camera view is not painted)
    const Bracket prof(&h->prof);
    hipError_t e;
    if ((e = prof.mark(0, h->stream)) != hipSuccess) return e;
    if ((e = rcw_launch_cast(h->dev, actions_dev, mask_dev, h->stream)) != hipSuccess) return e;
    h->step.columns_cast(mask_dev != nullptr);
    // (RCW_VIEW_ONLY: nothing is rendered yet — the source's kernel and the restarted agents' cast go right here, and the top view and the
    // view kernel below render every agent once; the two launches count into cast_ms of a handle that has a source)
    if (restarts && ((e = launch_layout_source(h, false)) != hipSuccess || (e = launch_start_distance(h, false)) != hipSuccess ||
                     (e = rcw_launch_cast(h->dev, nullptr, restarted, h->stream)) != hipSuccess)) return e;
    if ((e = prof.mark(1, h->stream)) != hipSuccess) return e;
    if (h->dev.top_view && (e = launch_top_view_alone(h, mask_dev)) != hipSuccess) return e;
    if ((e = prof.mark(2, h->stream)) != hipSuccess) return e;
    if ((e = launch_view(h, mask_dev, op)) != hipSuccess) return e;
    if ((e = prof.done(h->stream)) != hipSuccess) return e;
    if ((e = launch_goal_distance(h, mask_dev, op)) != hipSuccess) return e;
    if ((e = launch_guide(h, op)) != hipSuccess) return e;
    if ((e = launch_seen_map(h, mask_dev, op)) != hipSuccess) return e;
    if ((e = launch_frontier(h, mask_dev, op)) != hipSuccess) return e;
    if ((e = launch_visit_map(h, mask_dev, op)) != hipSuccess) return e;
    if ((e = launch_local_map(h, op)) != hipSuccess) return e;
    return launch_episode_stats(h, mask_dev, op);
}

// A save or a restore of the state archive, on the handle's stream and without a wait (the caller has checked that the handle's shape is the
// archive's: every segment has its live array).  Both: who takes which row, then the copy — the segment table goes to the kernel
// kSnapshotKernelSegments at a time.  A save is done there.  A restore goes on: the step's facts forget the slots (StepFacts::restored), and
// the agents of the mask are cast and painted from the state they now hold, as a re-render of the same frames is (kStackKeep): the flood, the
// seen map, the visit map, the stack, the local map and the statistics are the record's and stay as the gather left them.  The guide's words are no part
// of the record: its kernel follows, on the restored state.  Nor is anything of the frontier: the agents of the mask are flooded again
// from the seen map the gather restored, and the action words of every agent follow.
hipError_t launch_snapshot(rcw_handle* h, const int32_t* rows_dev, const uint8_t* mask_dev, bool restore)
{
    rcw_handle::Snapshots& sn = h->snaps;
    hipError_t e;
    if (!restore && (e = hipMemsetAsync(sn.owner, 0xFF, (size_t)sn.rows * sizeof(int32_t), h->stream)) != hipSuccess) return e;   // (-1: nobody)
    if ((e = rcw_launch_snapshot_resolve(h->dev, h->B, rows_dev, mask_dev, sn.rows, restore, sn.filled, sn.owner, sn.sel, h->stream)) != hipSuccess) return e;
    for (int first = 0; first < sn.plan.n; first += kSnapshotKernelSegments) {
        RcwSnapshotTable t{};
        for (int k = first; k < sn.plan.n && t.n < kSnapshotKernelSegments; ++k) {
            const LiveArray& live = h->live[sn.plan.seg[k].field];     // (the array the segment is a copy of: of the segment's size, or nothing is copied)
            if (!live.ptr || live.bytes != sn.plan.seg[k].bytes) return hipErrorInvalidValue;
            t.seg[t.n++] = RcwSnapshotSeg{live.as<uint8_t>(), sn.arc[k], sn.plan.seg[k].bytes, t.tasks};
            t.tasks += rcw_snapshot_tasks(sn.plan.seg[k].bytes, h->B);
        }
        if ((e = rcw_launch_snapshot_copy(t, h->B, sn.sel, restore ? nullptr : sn.owner, restore, 8 * h->hw.cus, h->stream)) != hipSuccess) return e;
    }
    if (!restore) return hipSuccess;
    h->step.restored();
    if ((e = launch_step(h, nullptr, mask_dev, kStackKeep)) != hipSuccess) return e;
    if ((e = launch_guide(h, kStackRefill)) != hipSuccess) return e;   // (no part of the record: computed from the restored field, pose and the table as it is now)
    return launch_frontier(h, mask_dev, kStackRefill);
}

// THE way a buffer of a live handle is given up: wait_all_streams (queued work may still use the old ones), then each of `old` takes
// over its partner in `fresh` (allocated by the caller beforehand, where the old one must survive a failure) or, without one, is dropped.
hipError_t replace_buffers(rcw_handle* h, std::initializer_list<RcwBuf*> old, std::initializer_list<RcwBuf*> fresh)
{
    const hipError_t e = wait_all_streams(h);
    auto f = fresh.begin();
    if (e == hipSuccess) for (RcwBuf* q : old) *q = f != fresh.end() ? std::move(**f++) : RcwBuf();
    return e;
}

// Which form update_top_view! (SR:446-483) takes for this handle (top_view_rule), and its scratch in HBM.
int plan_top_view(rcw_handle* h, int want_form, int want_runs, bool lenient)
{
    RcwPlan& d = h->dev;
    const size_t B = (size_t)h->B;
    RCW_HIP(replace_buffers(h, {&h->d_top_plane, &h->d_top_hdr, &h->d_top_codes}));
    d.top_plane = nullptr; d.top_hdr = nullptr; d.top_codes = nullptr;
    int rc = top_view_rule(d, &h->cfg, B, h->hw, want_form, want_runs, lenient);
    if (rc != RCW_OK || !h->cfg.render_top_view) return rc;
    if (d.top_split) {
        hipError_t e = h->d_top_plane.hipMalloc(rcw_top_plane_bytes(d));
        // The planes start out ZERO.  The flat store kernel ORs the plane words of two neighbouring agents' regions in a chunk
        // that holds pixels of both and relies on a region's bits outside its own image being zero — true of every region the
        // draw kernel has written, but a masked render right after rcw_set_top_view_form (whose own re-render may be the
        // one-kernel form, which writes no planes) draws the masked agents only and reads their neighbours' regions as they lie.
        // (stream-ordered on the handle's stream: every later launch of the handle comes behind it, the side stream's draw
        // kernel through the fork event)
        if (e == hipSuccess) e = hipMemsetAsync(h->d_top_plane.get(), 0, rcw_top_plane_bytes(d), h->stream);
        if (e == hipSuccess) e = h->d_top_hdr.hipMalloc((size_t)h->B * sizeof(int2));
        if (e == hipSuccess) e = hipMemsetAsync(h->d_top_hdr.get(), 0, (size_t)h->B * sizeof(int2), h->stream);
        if (e == hipSuccess) e = h->d_top_codes.hipMalloc(rcw_top_codes_bytes(d));
        if (e == hipSuccess && !h->top_stream.get()) e = h->top_stream.hipStreamCreate();
        if (e == hipSuccess && !h->ev_top_fork.get()) e = h->ev_top_fork.hipEventCreate(hipEventDisableTiming);
        for (RcwEvent& q : h->ev_top_join) if (e == hipSuccess && !q.get()) e = q.hipEventCreate(hipEventDisableTiming);
        if (e != hipSuccess) return fail(hip_code(e), "top view planes: %s", hip_failure(e));
        d.top_plane = h->d_top_plane.get<uint32_t>(); d.top_hdr = h->d_top_hdr.get<int2>(); d.top_codes = h->d_top_codes.get<uint2>();
    }
    hipError_t e = rcw_prepare_top_view(d, h->device);
    if (e != hipSuccess) return fail(RCW_ERR_HIP, "top view kernel attribute: %s", hip_failure(e));
    return RCW_OK;
}

// Which form a step takes (rcw_set_step_form; want = 0: the rule — one launch where the geometry allows AND the batch is large enough
// for it to pay, unless a step of the handle was captured into a graph).  Allocates the two slot buffers the first time the one-launch
// form is taken; the caller primes them (launch_step without an action).
int plan_step_form(rcw_handle* h, int want)
{
    const RcwPlan& d = h->dev;
    rcw_handle::Step& st = h->step;
    const StepFacts::Plan p = st.plan(want, h->learner.only(), rcw_step_spec_eligible(d) != 0, step_one_launch_pays(d));
    if (p.refused) return fail(RCW_ERR_UNSUPPORTED, "%s", p.refused);
    for (RcwBuf& q : st.slot) {
        if (!p.on || q.get()) continue;
        const hipError_t e = q.hipMalloc(rcw_step_spec_slot_bytes(d));
        if (e != hipSuccess) return fail(hip_code(e), "one-launch step, slot buffers: %s", hip_failure(e));
    }
    st.take(p);
    return RCW_OK;
}

// The descriptors of the current frames, where the one-launch step left them stale (StepFacts::cols_live): cast_rays! SR:195-231 on the
// current state, no action — the cast kernel, stream-ordered in front of the reader.
int ensure_columns(rcw_handle* h)
{
    if (!h->step.cols_stale()) return RCW_OK;
    RCW_HIP(rcw_launch_cast(h->dev, nullptr, nullptr, h->stream));
    h->step.columns_cast();
    return RCW_OK;
}

// The one teardown (rcw_destroy, and a failed rcw_create through its unique_ptr): nothing is freed before all three streams were waited
// for (a failed wait is ignored: the handle goes either way); the members follow in reverse order of declaration, the streams last.
rcw_handle::~rcw_handle()
{
    (void)hipSetDevice(device);
    (void)wait_all_streams(this);
    drop_comm(this);
}
