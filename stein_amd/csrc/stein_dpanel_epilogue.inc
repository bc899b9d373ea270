// stein_dpanel_epilogue.inc -- the epilogue of one strip of k_distance_panel / k_distance_panel_deep, included textually by
// both kernels (one source for the code that defines what D holds; a function would take twenty reference parameters).
// In scope at the point of inclusion: SYM, D, ntc, I, cfirst, members, s (the strip), acc[8][2], rj[2], nts, stg, window,
// sx, hist, hx, lane, li, lq, and DP_RI(ib) = the norm of row 16 ib + li of the row tile.  Leaves `diag` (the strip lies in the row tile's diagonal tile) defined for the code behind it.
        const int c32 = cfirst + members * s;
        float* __restrict__ dt = D + ((size_t)I * ntc + c32) * DT_ELEMS;
        const bool diag = SYM && (c32 >> 2) == I;
        const u32 wt = SYM ? 2u : 1u;
        // a strip of the diagonal tile stores entry by entry behind the same staging: (i, j) for i <= j and, for i < j, the
        // same value at its mirror place (j, i); the entries below the diagonal belong to the strip that holds their mirror
        const int d4 = c32 & 3;
        float* __restrict__ dmir = D + ((size_t)I * ntc + 4 * I) * DT_ELEMS;      // the diagonal tile's first 32 columns
        const int sr = lane >> 3, sc4 = (lane & 7) * 4;                          // staged row / first column of this lane
        const int lane_dir = sr * 32 + sc4, lane_dij = sr - sc4;                  // (staged-row layout: direct stores)
        const int lane_mir = lq * 128 + li, lane_dji = 4 * lq - li;               // (accumulator layout: mirror stores)
        if (hist && !diag) {
          if (DP_HIST_EVERY == 1 || !hx.have) {   // the slots cover the digits around the first value this wave produces (any value will do)
            const u32 d0 = (u32)__builtin_amdgcn_readfirstlane((int)(__float_as_uint(__builtin_fmaf(acc[0][0][0], nts, DP_RI(0) + rj[0][0])) >> 21));
            hx.base = d0 >= 1024u ? 0u : (d0 < 3u ? 0u : (d0 - 3u > 1016u ? 1016u : d0 - 3u));
            hx.have = true;
          }
          hx.nacc += 1u;
        }
#ifdef DP_EPI_FAST
        // Regular strips (all but the four of a row tile's diagonal tile): one copy of the loop per mode -- plain, window,
        // histogram -- chosen by ONE branch per strip, the two column blocks of a 16-row block handled together.  In the generic
        // loop below every group of four entries asks "window? histogram? diagonal?" again: ~64 branches per strip, each worth
        // ~16 cycles next to the other wave's MFMAs, and the counting of a group could not start before the previous group's
        // LDS round trip had been waited for (stamps, round 4: epilogue 7.4 k of a strip's 21 k cycles with a window).
        if (!diag && window) {
          auto regular_strip = [&](auto mode) {
            constexpr int MODE = decltype(mode)::value;   // 0 plain, 1 window, 2 level-0 histogram
            // The staged rows of block ib are stored while block ib + 1 is being computed: a wave's LDS operations complete in
            // order, so the store of block ib waits for ITS two reads only (lgkmcnt counts down past them while the writes and
            // reads of block ib + 1 are still in the queue -- behind the other waves' fragment reads, ~1 k cycles at times).
            float4 px0, px1;
#pragma unroll
            for (int ib = 0; ib < 8; ++ib) {
              float v[2][4];
              const float rib = DP_RI(ib);
              // (NOT v_pk_add_f32 / v_pk_fma_f32, two entries per instruction: the packed fp32 instructions go through the
              // matrix pipe's issue path and starve while the SIMD's other wave is in its MFMA loop -- one every ~256 cycles
              // against one plain VALU instruction every ~10, scratch/coissue_probe.hip)
#pragma unroll
              for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[jb][e] = __builtin_fmaf(acc[ib][jb][e], nts, rib + rj[jb][e]);
              if (MODE == 1) dp_count8(sx, v, wt, lane);
              if (MODE == 2) { dp_hist4(hx, v[0]); dp_hist4(hx, v[1]); }
#pragma unroll
              for (int jb = 0; jb < 2; ++jb)
                *reinterpret_cast<float4*>(stg + li * DP_PITCH + jb * 64 + lq * 16) = make_float4(v[jb][0], v[jb][1], v[jb][2], v[jb][3]);
              const float4 x0 = *reinterpret_cast<const float4*>(stg + sr * DP_PITCH + sc4 * 4);
              const float4 x1 = *reinterpret_cast<const float4*>(stg + (8 + sr) * DP_PITCH + sc4 * 4);
              if (ib > 0) {
                *reinterpret_cast<float4*>(dt + (ib - 1) * 512 + lane * 4) = px0;          // rows 16 (ib - 1) .. + 7: 1 KB contiguous
                *reinterpret_cast<float4*>(dt + (ib - 1) * 512 + 256 + lane * 4) = px1;    // rows 16 (ib - 1) + 8 .. + 15
              }
              px0 = x0; px1 = x1;
            }
            *reinterpret_cast<float4*>(dt + 7 * 512 + lane * 4) = px0;
            *reinterpret_cast<float4*>(dt + 7 * 512 + 256 + lane * 4) = px1;
          };
          regular_strip(std::integral_constant<int, 1>{});
        } else
#endif
#pragma unroll
        for (int ib = 0; ib < 8; ++ib) {
#pragma unroll
          for (int jb = 0; jb < 2; ++jb) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(acc[ib][jb][e], nts, DP_RI(ib) + rj[jb][e]);
            if (window && !diag) { const u32 w4[4] = {wt, wt, wt, wt}; dp_count4<true>(sx, v, w4, wt, lane); }
            if (hist && !diag) dp_hist4(hx, v);
            *reinterpret_cast<float4*>(stg + li * DP_PITCH + jb * 64 + lq * 16) = make_float4(v[0], v[1], v[2], v[3]);
            if (diag && ib < 2 * d4 + 2) {
              // mirror places, straight from the accumulator layout: lane = row i, so the 16 lanes of a quarter wave write 64
              // contiguous bytes of mirror row j.  (From the staged rows, where neighbouring lanes hold neighbouring COLUMNS,
              // every lane's 4 bytes were a memory transaction of their own: ~8000 per strip, ~150 us, during which the
              // other waves of the CU could not issue their loads either.)
              const int dji = 32 * d4 + 16 * jb - 16 * ib + lane_dji;               // j - i at e = 0
              float* __restrict__ pm = dmir + (size_t)(ib >> 1) * DT_ELEMS + (d4 * 32 + jb * 16) * 32 + ((16 * ib) & 31);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (dji + e > 0) pm[lane_mir + e * 32] = v[e];
            }
          }
          const float4 x0 = *reinterpret_cast<const float4*>(stg + sr * DP_PITCH + sc4 * 4);
          const float4 x1 = *reinterpret_cast<const float4*>(stg + (8 + sr) * DP_PITCH + sc4 * 4);
          if (!diag) {
            *reinterpret_cast<float4*>(dt + ib * 512 + lane * 4) = x0;          // rows 16 ib .. + 7: 1 KB contiguous
            *reinterpret_cast<float4*>(dt + ib * 512 + 256 + lane * 4) = x1;    // rows 16 ib + 8 .. + 15
          } else if (ib < 2 * d4 + 2) {                                          // (blocks below the diagonal block: nothing)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const float xs[4] = {h ? x1.x : x0.x, h ? x1.y : x0.y, h ? x1.z : x0.z, h ? x1.w : x0.w};
              // row i = i0 + sr and column j = 32 d4 + sc4 + e inside the tile; everything but lane_dir / dij is
              // wave-uniform (addresses written out this way keep the diagonal path to a handful of registers)
              const int i0 = 16 * ib + 8 * h;
              float* __restrict__ pd = dt + i0 * 32;
              const int dij = i0 - 32 * d4 + lane_dij;                           // i - j at e = 0
              u32 w4[4];
              // the lane's four columns lie all above the diagonal (one 16-byte store, as everywhere else), all below it
              // (nothing), or straddle it (entry by entry; a handful of lanes).  Sixty-four single-entry stores 16 bytes apart
              // per instruction made a diagonal strip take ~100 us: the waves that drew them held up their whole team.
              if (dij < 0) *reinterpret_cast<float4*>(pd + lane_dir) = make_float4(xs[0], xs[1], xs[2], xs[3]);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                w4[e] = dij < e ? 2u : (dij == e ? 1u : 0u);
                if (w4[e] && dij >= 0) pd[lane_dir + e] = xs[e];
              }
              if (window) dp_count4<false>(sx, xs, w4, 0u, lane);
              if (hist) {   // a diagonal strip: per-entry weights, straight into the workgroup's histogram
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (w4[e]) atomicAdd(&hx.hl[dp_key_digit(__float_as_uint(xs[e]) >> 21)], w4[e]);
              }
            }
          }
        }
        // 8-bit slots: at most 3 x 64 entries per lane between flushes (DP_HIST_EVERY = 1 in the deep kernel: the slots then
        // are dead across its K loop, where every register is spoken for)
        if (DP_HIST_EVERY == 1) { if (hist && !diag) { hx.nacc = 1u; dp_hist_flush(hx, lane); } }
        else if (hist && hx.nacc >= (u32)DP_HIST_EVERY) dp_hist_flush(hx, lane);
