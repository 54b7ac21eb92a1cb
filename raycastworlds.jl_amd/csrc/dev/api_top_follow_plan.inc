// Development build only (-DRCW_DEV_SWITCHES): RCW_TOP_FOLLOW — the counters' block size and where the store kernel may follow the draw kernel.  A fragment of rcw_api.hip (plan_top_view), included where it stood.
        d.top_flags = h->d_top_flags.get<uint32_t>();
        while ((((size_t)h->B + ((size_t)1 << d.top_blk_shift) - 1) >> d.top_blk_shift) > 1024) ++d.top_blk_shift;   // at most 1024 blocks: sixteen looks of a wavefront see them all
        // the store kernel follows the draw kernel (no event between them) where their workgroups fit on a CU together:
        // bit 0 inside a step (side-stream form, one run), bit 1 in rcw_update_top_view alone
        d.top_follow_ok = (!d.top_fused && d.top_runs <= 1 && rcw_top_follow_fits(d, d.top_draw_block, true, h->hw.cus) ? 1 : 0) |
                          (d.top_alone_split && rcw_top_follow_fits(d, d.top_draw_block_alone, false, h->hw.cus) ? 2 : 0);
        { const char* v = RCW_DEV_ENV("RCW_TOP_FOLLOW"); d.top_follow_ok &= v ? std::atoi(v) : 0; }   // (off unless asked for)
        if (d.top_draw_r4 || d.top_parts > 1) d.top_follow_ok = 0;
