// The full-tile k loops and the tail of gemm_f32_kernel's one-tile-prefetch (DEEP == 0) form, behind the prologue and the
// convolution loop: included by gemm_f32.hip inside the kernel, twice.
// VQA_KLOOPS_GS: this workgroup copies every staged A tile to gathered_out (row-gathered kernels, column panel 0,
// by-product requested).  The offset form of the row-gathered kernel takes it as the constants true and false, i.e.
// two copies of the loops chosen once per output tile: one copy with a workgroup-uniform `if` around the by-product
// stores cost EVERY workgroup 27 us of the bench GEMM's 536, whether it took the branch or not
// (profiles/r22_gather_gemm.txt).  Every other kernel sees false (or, the pointer form, the test itself) in one copy.
        if (!CONV && !EDGE) {
            // full tiles, two per trip so both LDS buffers are compile-time addresses
            if (!GATHER) sa.init_full(p.lda, m0, kbeg, p.M);      // (row-gathered: the offsets are set above)
            sb.init_full(p.ldb, n0, kbeg, p.N);
            const unsigned stepA = (unsigned)(A_KC ? BK : BK * p.lda) * 4u;
            const unsigned stepB = (unsigned)(B_KC ? BK : BK * p.ldb) * 4u;
            const int nfull = (kend - kbeg) / BK;
            unsigned oa = stepA, ob = stepB;   // scalar byte offsets of tile t + 1
            // fetch_ab: the next tile (at oa / ob) into the staging registers; put_g: the by-product copy of the A tile
            // in the staging registers, which is the one fetch_ab fetched last
            auto fetch_ab = [&](int tile) {      // (the pointer form takes the tile number: two tiles of one trip then differ by an immediate)
                if (GATHER == 1) sa.load_ptr(gsrc, tile * BK); else sa.load_full(rsA, oa);
                sb.load_full(rsB, ob);
                oa += stepA; ob += stepB;
            };
            auto put_g = [&]() { if (VQA_KLOOPS_GS) sa.store_buf(rsG, gdst, oa - stepA); };
            // Stagger (8-wave workgroups: waves w and w + 4 share a SIMD and, running the same program with one
            // barrier per k tile, reach their MFMA burst, their LDS traffic and the barrier together).  Inside one
            // barrier interval "compute tile t from one LDS buffer" and "store tile t+1 into the other" commute, so
            // waves 4..7 run the interval as store(t+1) -> fetch(t+2) -> compute(t) while waves 0..3 keep
            // fetch(t+1) -> compute(t) -> store(t+1): a SIMD's two waves of this workgroup alternate between the
            // MFMA burst and the LDS/global phase instead of colliding in both.  Same barrier count on both paths;
            // one entry fetch and one transition interval bring waves 4..7 in and out of the half-interval lead.
            // Compiled in only where it pays and costs no occupancy: the 128x64 / 64x128 tiles of 32x32 waves with BK 32
            // (95 -> 99 registers, still two workgroups per CU) and the 128x128 BK-16 weight-gradient tile; in the
            // 128x128 BK-32 kernel the second loop body costs 6 registers and with them its second workgroup per CU
            // (124 -> 130: the extractor's 1x1 layers lost 1.3 % until this was fenced off).
            constexpr bool STAG = (NT == 512) && GATHER != 1 && EPI == EPI_PLAIN && (VQA_GEMM_STAGGER != 0) &&
                                  ((WM == 32 && WN == 32 && BK == 32 && BM + BN == 192) || (BM == 128 && BN == 128 && BK == 16));
            // Long k loops only: on the roofline GEMM (64 tiles) the k loop gets 2 % shorter (552 -> 541 us, same
            // box, two builds); on the extractor's short-k 1x1 layers (4..8 tiles) the entry fetch and the transition
            // interval cost more than the stagger returns (2064 -> 2043 imgs/s).  profiles/r2_stagger_ab.txt
            const bool stag_wg = STAG && nfull >= 16;                 // workgroup-uniform
            if (stag_wg && wave >= 4) {
                // (a static s_setprio 1 for this second-dispatched half, the guide's companion rule, made the roofline
                // GEMM 2 % SLOWER here: 563 -> 574 us, same box, two builds)
                fetch_ab(1);                                           // tile 1 into the staging registers
                for (; t + 3 < nfull; t += 2) {
                    sa.store(L1); sb.store(L1 + A_FL); put_g();       // tile t + 1
                    fetch_ab(t + 2);                                       // tile t + 2
                    __builtin_amdgcn_sched_barrier(0);
                    compute_tile(L0, L0 + A_FL);
                    __builtin_amdgcn_sched_barrier(0);
                    __syncthreads();
                    sa.store(L0); sb.store(L0 + A_FL); put_g();       // tile t + 2
                    fetch_ab(t + 3);                                       // tile t + 3
                    __builtin_amdgcn_sched_barrier(0);
                    compute_tile(L1, L1 + A_FL);
                    __builtin_amdgcn_sched_barrier(0);
                    __syncthreads();
                }
                sa.store(L1); sb.store(L1 + A_FL); put_g();           // transition: tile t + 1 (< nfull) is in the registers
                __builtin_amdgcn_sched_barrier(0);
                compute_tile(L0, L0 + A_FL);
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                ++t;
            } else if (stag_wg) {
                for (; t + 3 < nfull; t += 2) {                       // the same trip count as the waves above
                    fetch_ab(t + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    compute_tile(L0, L0 + A_FL);
                    __builtin_amdgcn_sched_barrier(0);
                    sa.store(L1); sb.store(L1 + A_FL); put_g();
                    __syncthreads();
                    fetch_ab(t + 2);
                    __builtin_amdgcn_sched_barrier(0);
                    compute_tile(L1, L1 + A_FL);
                    __builtin_amdgcn_sched_barrier(0);
                    sa.store(L0); sb.store(L0 + A_FL); put_g();
                    __syncthreads();
                }
                if (GATHER == 1) sa.load_ptr(gsrc, (t + 1) * BK); else sa.load_full(rsA, oa);       // transition interval
                sb.load_full(rsB, ob);
                __builtin_amdgcn_sched_barrier(0);
                compute_tile(L0, L0 + A_FL);
                __builtin_amdgcn_sched_barrier(0);
                sa.store(L1); sb.store(L1 + A_FL);
                if (VQA_KLOOPS_GS) sa.store_buf(rsG, gdst, oa);
                __syncthreads();
                ++t;
            }
            for (; !stag_wg && t + 2 < nfull; t += 2) {
                fetch_ab(t + 1);
                __builtin_amdgcn_sched_barrier(0);
                compute_tile(L0, L0 + A_FL);
                __builtin_amdgcn_sched_barrier(0);
                sa.store(L1);
                sb.store(L1 + A_FL);
                put_g();
                __syncthreads();
                fetch_ab(t + 2);
                __builtin_amdgcn_sched_barrier(0);
                compute_tile(L1, L1 + A_FL);
                __builtin_amdgcn_sched_barrier(0);
                sa.store(L0);
                sb.store(L0 + A_FL);
                put_g();
                __syncthreads();
            }
        }
        // remaining tiles (all of them for the conv / edge loaders) without conditionals, the last
        // one peeled: loads of tile t+1 are issued before tile t's MFMA loop and consumed after it
        for (; t + 1 < nt; ++t) {
            float* cur = (t & 1) ? L1 : L0;
            float* nxt = (t & 1) ? L0 : L1;
            load_a(kbeg + (t + 1) * BK);
            load_b(kbeg + (t + 1) * BK);
            __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ABOVE the MFMA loop (hipcc sinks it otherwise)
            compute_tile(cur, cur + A_FL);
            __builtin_amdgcn_sched_barrier(0);
            sa.store(nxt);
            sb.store(nxt + A_FL);
            if (VQA_KLOOPS_GS) sa.store_buf(rsG, gdst, (unsigned)((t + 1) * BK) * 4u);
            __syncthreads();
        }
        if (nt > 0) {
            float* cur = ((nt - 1) & 1) ? L1 : L0;
            compute_tile(cur, cur + A_FL);
            __syncthreads();
        }
