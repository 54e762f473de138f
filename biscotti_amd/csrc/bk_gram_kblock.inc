// bk_gram_kblock.inc -- one k-block of g3_wave's ring loop (bk_gram.hip), included
// once per loop with `constexpr bool STEADY` set by the includer: true in the
// peeled loop whose every k-block still stages another (t + 2 < nk: no run-time
// "more", so the k-block is one basic block and the glds can be spread), false
// in the plain loop.  Plain text inclusion: wrapping the k-block in a lambda
// or a function changed the register allocation of every instance.
        const int ahead = STEADY ? G3_STAGES - 2 : min(nk - t - 1, G3_STAGES - 2);  // stages issued after t
        G3_PROBE(p0);
        if constexpr (NB > 0 && MODE != 2 && ESPL != 0) {
            if (ahead > 0)
                g3_waitc<WCNT>();
            else
                g3_waitc<0>();
        } else if constexpr (NB > 0 && MODE != 2) {
            if (ahead > 0)
                g3_waitc<(NB < BK_K1_GLDS_LIMIT ? NB : BK_K1_GLDS_LIMIT)>();
            else
                g3_waitc<0>();
        } else {
            g3_wait(MODE == 2 ? 0 : ahead * c);
        }
        G3_PROBE(p1);
        g3_barrier();
        G3_PROBE(p2);
        probe[0] += p1 - p0;
        probe[1] += p2 - p1;
        const char *ls = lds + buf * G3_STAGE;
        const int nbuf = buf == 0 ? G3_STAGES - 1 : buf - 1;  // (t + STAGES - 1) % STAGES
        const bool more = (STEADY || t + G3_STAGES - 1 < nk) && MODE != 2 && !NOHI;
        const int64_t nkb = kst + (int64_t)(t + G3_STAGES - 1) * kstr;
        buf = buf == G3_STAGES - 1 ? 0 : buf + 1;
        if constexpr (MODE == 1) {
            if (more) issue(nkb, nbuf);
            continue;
        }
        // STEADY: waves 4-7 keep theirs in one burst where the branch used to pin it
        constexpr bool PIN = STEADY && HI && CNT > 0;
        if constexpr (KIND == T_OFF) {
            gran a0[4], b0[4], a1[4], b1[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a0[q] = g3_frag<T>(ls + sA * G3_BLK, q, 0, rr, g);
#pragma unroll
            for (int q = 0; q < 4; ++q) b0[q] = g3_frag<T>(ls + sB * G3_BLK, q, 0, rr, g);
            if constexpr (STAG) {
                if (t > 0) off_mma_gran<T, XO>(acc.a, ha, hb, xacc);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) a1[q] = g3_frag<T>(ls + sA * G3_BLK, q, 1, rr, g);
#pragma unroll
            for (int q = 0; q < 4; ++q) b1[q] = g3_frag<T>(ls + sB * G3_BLK, q, 1, rr, g);
            if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
            if (more) issue(nkb, nbuf);
            if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
            off_mma_gran<T, XO>(acc.a, a0, b0, xacc);
            if constexpr (STAG) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ha[q] = a1[q];
                    hb[q] = b1[q];
                }
            } else {
                off_mma_gran<T, XO>(acc.a, a1, b1, xacc);
            }
        } else if constexpr (KIND == T_PAIR) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                gran a[4], b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = g3_frag<T>(ls + sA * G3_BLK, q, h, rr, g);
#pragma unroll
                for (int q = 0; q < 4; ++q) b[q] = g3_frag<T>(ls + sB * G3_BLK, q, h, rr, g);
                if (h == 0 && more) issue(nkb, nbuf);
                diag_mma_g<T, XP>(acc.a, a);
                diag_mma_g<T, XP>(acc.b, b);
            }
        } else if constexpr (KIND == T_DIAG1) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                gran a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = g3_frag<T>(ls + sA * G3_BLK, q, h, rr, g);
                if (h == 0 && more) issue(nkb, nbuf);
                diag_mma_g<T>(acc.a, a);
            }
        } else {
            if (more) issue(nkb, nbuf);
        }
        if constexpr (STEADY && !HI && CNT > 0 && KIND != T_NONE) {
            // one glds after every K MFMAs of this wave's k-block, each issue
            // under its own in-flight MFMA and its SIMD partner's
            constexpr int SUB2 = 2 * G3T<T>::SUB;  // MFMA k-steps per k-block
            constexpr int NM = KIND == T_OFF    ? (16 + (XO != 0 ? 1 : 0)) * SUB2
                               : KIND == T_PAIR ? (XP ? 18 : 20) * SUB2
                                                : 10 * SUB2;
            constexpr int K = (NM + CNT - 1) / (CNT > 0 ? CNT : 1);
#pragma unroll
            for (int q = 0; q < CNT; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, K, 0);  // MFMA
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read (the glds)
            }
        }
