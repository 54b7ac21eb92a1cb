// Development build only (-DRCW_DEV_SWITCHES): RCW_STEP_PIECES=2, the batch in two halves with the second cast beside the first fill.  A fragment of rcw_api.hip, included where it stood.
    if (h->step_pieces == 2 && !d.top_view && h->top_stream.get() && d.B >= 2) {
        // Development experiment (RCW_STEP_PIECES=2, docs/experiments.md): the batch in two halves, the second half's cast kernel on
        // the side stream BESIDE the first half's fill: cast(1) | fork | fill(1) ∥ cast(2) | join | fill(2).
        const int B1 = d.B / 2, B2 = d.B - B1;
        const long long cols1 = (long long)B1 * d.N;
        if ((e = rcw_launch_cast(d, actions_dev, mask_dev, h->stream, 0, B1)) != hipSuccess) return e;
        if ((e = hipEventRecord(h->ev_top_fork.get(), h->stream)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(h->top_stream.get(), h->ev_top_fork.get(), 0)) != hipSuccess) return e;
        e = rcw_launch_cast(d, actions_dev, mask_dev, h->top_stream.get(), B1, B2);
        const hipError_t rec = hipEventRecord(h->ev_top_join[0].get(), h->top_stream.get());
        if (prof && e == hipSuccess) e = hipEventRecord(ev[1].get(), h->stream);
        if (prof && e == hipSuccess) e = hipEventRecord(ev[2].get(), h->stream);
        if (e == hipSuccess) e = rcw_launch_fill(d, d.col_h, d.col_c, d.obs, cols1, mask_dev, h->stream);
        if (rec == hipSuccess) { const hipError_t w = hipStreamWaitEvent(h->stream, h->ev_top_join[0].get(), 0); if (e == hipSuccess) e = w; }
        if (e == hipSuccess) e = rec;
        if (e == hipSuccess)
            e = rcw_launch_fill(d, d.col_h + cols1, d.col_c + cols1, d.obs + cols1 * d.Hc, (long long)B2 * d.N, mask_dev ? mask_dev + B1 : nullptr, h->stream);
        if (e != hipSuccess) return e;
        if (prof) { if ((e = hipEventRecord(ev[3].get(), h->stream)) != hipSuccess) return e; h->prof_count++; }
        return hipSuccess;
    }
