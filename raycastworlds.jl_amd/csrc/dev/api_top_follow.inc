// Development build only (-DRCW_DEV_SWITCHES): RCW_TOP_FOLLOW, the launch order in which the store kernel follows the draw kernel.  A fragment of rcw_api.hip, included where it stood.
    // Development experiment (RCW_TOP_FOLLOW = 1 inside a step | 2 alone; measured slower, docs/experiments.md): the store kernel FOLLOWS
    // the draw kernel where that is safe (rcw_kernels.hip, top_publish): an unmasked whole batch, the two
    // kernels' workgroups fitting on a CU together (d.top_follow_ok), and no stream capture (a graph would replay this call's number,
    // and promises no concurrency between its branches).  The draw kernel goes to the side stream, the store kernel to the handle's
    // WITHOUT waiting for it — agent by agent it waits in memory —, and the handle's stream joins the side stream behind it.
    bool follow = mask_dev == nullptr && (d.top_follow_ok & (beside ? 1 : 2)) != 0 && !(beside && d.top_fused);
    if (follow) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(h->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) follow = false;
    }
    if (follow) {
        RcwDev dd = d;
        dd.top_epoch = ++h->top_epoch;                       // (the counters wrap with it: the comparison is modulo 2^32)
        dd.top_signal = 1; dd.top_follow = 1;
        if ((e = hipEventRecord(h->ev_top_fork.get(), h->stream)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(h->top_stream.get(), h->ev_top_fork.get(), 0)) != hipSuccess) return e;
        e = rcw_launch_top_draw(dd, nullptr, 0, d.B, h->top_stream.get(), beside ? 0 : d.top_draw_block_alone);
        const hipError_t rec = hipEventRecord(h->ev_top_join[0].get(), h->top_stream.get());
        if (e == hipSuccess) e = between(h->stream);
        if (e == hipSuccess) e = rcw_launch_top_store(dd, nullptr, 0, d.B, h->stream);
        if (rec == hipSuccess) { const hipError_t w = hipStreamWaitEvent(h->stream, h->ev_top_join[0].get(), 0); if (e == hipSuccess) e = w; }
        return e == hipSuccess ? rec : e;
    }
