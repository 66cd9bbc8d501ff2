// device_search_expansion.inc -- the text of search_kernel's expansion loop (device_search.h includes it where the loop
// stands; not a header of its own).  It is compiled with `ST` (steady copy) as a compile-time bool in scope and
// CPH_GO_STEADY defined as the statement that leaves the general copy for the steady one; everything else it names is
// search_kernel's local state.
        for (;;) {
            // ---- termination tests on the beam's top (:106-122); the pop itself comes later -----
            CPH_TICK(7);
            if constexpr (!ST && kTwoLoops) {
                // (num_slack <= 0: no schedule, the comparison holds from the start)
                if (nn_size >= k && slack_batch >= a.sc.num_slack - 1 && !(a.flags & 1u)) CPH_GO_STEADY;
            }
            if (beam_size == 0) break;
            uint32_t cur_id;
            float worst_pop;   // result-heap threshold as read here (wave-uniform)
            // std::pop_heap of the beam (whole wave while it lives in LDS, lane 0 once it has spilled)
            auto pop_beam = [&](uint32_t size) {
#ifdef CPH_TRAFFIC_STATS
                trf[5] += size;
                if (size > trf[6]) trf[6] = size;
                if (size > kBeamLds) { trf[0]++; uint32_t lv = 31u - (uint32_t)__builtin_clz(size); trf[1] += (lv - 7 + 4) / 5; }
                if (size > 8191) trf[7]++;
#endif
                if (size > 1) {
                    if (size <= kBeamLds) heap_pop_wave(heap, size, lane);
                    else beam_pop_hybrid(heap, size, lane);
                }
            };
            {
                const uint4 topv = heap.lds(0);
                const float worst = nn[0].dist;       // FLT_MAX while the result heap is empty (set at query start)
                cur_id = bcast_u32(topv.z);
                const float cur_est = __uint_as_float(topv.x);
                const float cur_lower = __uint_as_float(topv.y);
                // Every lane read the same words: the votes make the two decisions provably uniform.  (They were one
                // integer verdict -- 0 done, 1 pruned, 2 expand -- broadcast and tested twice; the compiler merged that
                // with the loop's other exits into a state word that the usual expansion tested again between the
                // verdict and its first load, and once more on the back edge.)
                const bool full = ST || nn_size >= k;
                if (any64(full && cur_est >= gamma_q * worst)) break;          // done
                if (any64(full && cur_lower > worst)) {                          // pruned: the entry leaves the beam, nothing is loaded
                    pop_beam(beam_size);
                    --beam_size;
                    continue;
                }
                worst_pop = bcast_f32(worst);
            }
            CPH_TICK(0);

            // ---- this expansion's loads, then the estimated-set probe (:227), a dependent round
            // trip that overlaps the exact distance and the result-heap push below ------------
            // (compile-time layout for the probe-first instantiations -- cph_core.h StaticLayout: they re-read the layout from
            // the kernarg segment inside the loop otherwise; the instantiations without it keep it in scalar registers, and
            // lose their clean loop -- two scratch reloads in the pop -- when the constants change the allocation)
            constexpr bool kStaticLayout = SD >= 128 && PF;
            const uint32_t blk_stride = kStaticLayout ? StaticLayout<BW, SD>::kStride : a.L.stride;
            const uint32_t blk_ids_off = kStaticLayout ? StaticLayout<BW, SD>::kIdsOff : a.L.ids_off;
            const uint8_t* blk = a.blocks + (size_t)cur_id * blk_stride;
            const float* vrow = a.raw + (size_t)cur_id * D;
            // Nothing that matters is in flight here (the previous expansion's prefetch is thousands
            // of cycles old, its marking atomics return nothing).  Saying so with a wait the compiler
            // can see keeps it from protecting registers it believes some path around the loop left
            // a load pending on -- such a wait, between the loads below, would be a real one.
#ifndef CPH_NO_LOOPHEAD_WAIT
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
#endif
            // The popped vertex's own vector goes straight to LDS (LDS-DMA, 16 B per lane, one
            // instruction for the 512 B; the strided per-chain reads then come from LDS).  It is
            // issued FIRST: loads retire in order, so retiring the other loads below also covers it.
            if constexpr (SD == 128) {
                if (lane < 32) lds_dma16(vrow + 4 * lane, vec_off);
                __builtin_amdgcn_sched_barrier(0);
            } else if constexpr (SD > 128) {
#pragma unroll
                for (int c = 0; c < SD / 256; ++c) lds_dma16(vrow + 4 * lane + 256 * c, vec_off + 1024 * c);
                __builtin_amdgcn_sched_barrier(0);
            }
            const float norm_ld = a.norm_sq[cur_id];
            const uint32_t nid_ld = reinterpret_cast<const uint32_t*>(blk + blk_ids_off)[li];
            // filtered: the popped vertex's allowed bit travels with the norm (retired with the block's loads below)
            uint32_t allow_cur = 0;
            if constexpr (FTAB) allow_cur = allow_q[cur_id >> 5];
            else if constexpr (FILT) allow_cur = CPH_COLD(allow)[cur_id >> 5];
            // ---- everything else this expansion reads is issued before the probe ----------
            BlockLoads<BW, SD> bl;
            // PROBE FIRST (the static-D instantiations, D = 128 and D = 1024; 4-bit codes at D = 128 in round 3, every width and
            // both shapes since round 4 -- the host picks the instantiation per workload).  The reference evaluates all 32 neighbours of a block, but only the NEW ones
            // -- 3.3 of 32 on the SIFT-like benchmark, none in a quarter of the expansions -- have any observable effect.  The
            // ids (128 B) decide that, so they, the norm and the vector go out here; the codes and aux values -- 2,560 of the
            // block's 2,752 bytes -- are fetched after the probe, by the lanes of the new neighbours only (both lane halves
            // of a neighbour; eight neighbours share a 128-byte line, so ~40 % of the lines drop out) and not at all when
            // nothing is new.  One more dependent round trip in three expansions out of four against ~40 % less traffic:
            // full queue 16.4 -> 15.3 ms per 100,000 queries, the 10,000-query launch 2.19 -> 2.14 ms, results identical.
            // Whether it pays depends on how many neighbours are new: on the SIFT-like data (1-3 of 32) it gains 7-13 % at
            // every bit width, on the Gaussian gate workloads (5-10 new, nothing to skip) it only adds a round trip (-3 % to
            // -13 %): the library chooses from the previous batches' own counters (cphnsw_mi355x.hip: probe_first).  Without
            // it the narrow codes run their estimator under the probe's round trip (kSpeculate).
#ifdef CPH_NO_PROBE_FIRST
            constexpr bool kProbeFirst = false;
#else
            constexpr bool kProbeFirst = PF && SD >= 128;
#endif
            if constexpr (!kProbeFirst) bl.issue(blk, a.L, lane);
            __builtin_amdgcn_sched_barrier(0);
            CPH_TICKF(0);
            // ---- the pop, while those loads are in flight.  It needs only the id of the top, which the loads
            // above already have; its three dependent LDS round trips and its scalar path walk (a fifth of an
            // expansion's time when it ran in front of the loads) now hide behind the block's memory latency.
            // LDS and scalar work only (lgkmcnt), so no wait on the loads (vmcnt) is forced here.
            // Spilled beams: the pushes at the end of this expansion will compare against the ancestors of the leaf the
            // pop is about to free (heap index beam_size - 1).  Those of them that live in the pages are touched now, one
            // per lane, in the same round trip as the block: the pushes' own reads then hit in L2 instead of being another
            // dependent trip to HBM.  The value is consumed, unused, where the block's loads are retired anyway (the touch
            // is the youngest load there, so the compiler's wait for it is the wait the block needs in any case); beams
            // that fit the LDS levels -- every C2 expansion -- skip the whole thing on a wave-uniform branch.
            uint32_t touch = 0;
            if (beam_size > kBeamLds) {
                // leaf = heap index beam_size - 1, i.e. hp = beam_size on level `depth`; its ancestor on level 7 + j
                // (j = 1..5, below the leaf's own level) is relative node ((hp >> (depth - 7 - j)) & (2^j - 1)) | 2^j
                // of the page of hp >> (depth - 7): lane j - 1 touches it
                const uint32_t depth = 31u - (uint32_t)__builtin_clz(beam_size);
                const uint32_t j = (uint32_t)lane + 1u;
                const bool on = j <= 5u && 7u + j < depth;
                const uint32_t sh = on ? depth - 7u - j : 0u;
                const uint32_t rj = ((beam_size >> sh) & ((1u << (j & 7u)) - 1u)) | (1u << (j & 7u));
                const uint32_t pb = ((beam_size >> (depth - 7u)) - 128u) * kPageDwords;
                touch = heap.gp[on ? pb + 3u * rj : 0u];
            }
            pop_beam(beam_size);
            --beam_size;
            __builtin_amdgcn_sched_barrier(0);
            CPH_TICKF(1);
            // All of this expansion's loads come back together (issued back to back, retired in
            // order); they are retired HERE, before the probe goes out.  The probe is only issued when
            // a lane has something to look up, and a load that is only maybe in flight makes every
            // later wait of the compiler a vmcnt(0) -- the norm or the codes would then wait for the
            // probe's round trip.  This way that round trip (and the prefetch behind it) overlaps the
            // whole estimator arithmetic; the vector DMA is older than these loads, so it has landed.
            uint32_t nid = nid_ld;
            float cur_norm = norm_ld;
            float dot_generic = 0.0f;
            if constexpr (SD < 128) dot_generic = bcast_f32(group_dot8_lo(qv, vrow, D, lane & 7));   // its loads, too, go first
            if constexpr (!kProbeFirst) bl.retire();
            asm volatile("" : "+v"(cur_norm), "+v"(nid) : "v"(touch));
            CPH_TICKF(2);
            const bool valid = nid != kInvalidNode;  // slot < count (set by the repacker)
            const bool active = lane < 32 && valid;
            // The probe is a plain (device-coherent: it must not be served from this CU's L1, which
            // the marking atomics below bypass) load of the slot's bitmap word; only the few
            // neighbours that turn out to be new pay for a read-modify-write, and that one needs
            // no return value.  (A test-and-set for all 32 made the L2 atomic units the bottleneck.)
            uint32_t old_bits = 0;
            const uint32_t my_bit = 1u << (nid & 31);
            // (every lane loads -- the upper half and empty slots read word 0 -- instead of a predicated load: one select
            // against an exec-mask save / branch / restore on the scalar unit)
            old_bits = __hip_atomic_load(&bm[active ? nid >> 5 : 0u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_sched_barrier(0);
#ifdef CPH_TRAFFIC_STATS
            {   // distinct 128-byte lines of the bitmap this probe touches
                const uint32_t line = nid >> 10;
                bool first = active;
                for (int j = 0; j < 31; ++j) {
                    const uint32_t oj = __shfl(line, j);
                    const bool aj = __shfl((int)active, j) != 0;
                    if (aj && lane > j && oj == line) first = false;
                }
                trf[4] += __popcll(ballot64(first));
            }
#endif

            // ---- exact distance of the popped node; nn.push (:130-133) ----------------
            float exact_dist;
            {
                float dot;
                if constexpr (SD >= 128) dot = bcast_f32(group_reduce8_lo(chain_dot_lds<SD / 8>(qv, s_vec, lane & 7, 0.0f)));
                else dot = dot_generic;
                exact_dist = exact_from_dot(qnorm, cur_norm, dot);
            }
            if constexpr (!kDerivedCounters) st_exact++;
            st_exp++;
            // BoundedMaxHeap::push changes the heap only while it is filling or when the new distance
            // beats the threshold: both are wave-uniform facts, so the three expansions out of four
            // that leave it alone skip the lane-0 section and the re-read of the threshold
            float worst0 = worst_pop;
            // (filtered: a vertex outside the allowed set never enters the result heap -- cur_id is uniform, so is this)
            const bool cur_allowed = !FILT || ((allow_cur >> (cur_id & 31u)) & 1u) != 0u;
            const bool nn_changes = any64(cur_allowed && ((!ST && nn_size < k) || exact_dist < worst_pop));   // every lane agrees: provably uniform
            if (nn_changes) {
                nn_push_wave<ST>(nnw, nn, nn_size, k, cur_id, exact_dist, worst_pop, lane);
                __builtin_amdgcn_wave_barrier();
                worst0 = bcast_f32(nnw.lds_key(0));   // (the heap holds at least the entry just pushed)
            }
            const uint32_t nn_sz = nn_size;
            CPH_TICK(1);
            CPH_TICKF(3);
            if (!any64(active)) {  // n_neighbors == 0 (:137)
                // (retire the probe's destination register on this path too: a load left pending
                // across the back edge costs every expansion a wait where that register is reused)
                asm volatile("" ::"v"(old_bits));
                continue;
            }

            // slack level schedule (:141-145); steady: the last level, set where the query changed loops
            if constexpr (!ST) {
                if (a.sc.num_slack > 0) {
                    int lvl = slack_batch < a.sc.num_slack - 1 ? slack_batch : a.sc.num_slack - 1;
                    qp.slack = s_slack[lvl];
                    ++slack_batch;
                }
            }
            // ---- FastScan estimates (:159-206) ----------------------------------------
            float est = 0.0f, lower = 0.0f;
            bool skipped2 = false, undecided2 = false;
            // a list shorter than 32 whose length is not a multiple of 8 ends in the reference's scalar tail
            // (device_fastscan.h: TailLanes); wave-uniform, never taken on graphs the builders write.  The probe-first
            // instantiation sits on its register limit and is only launched on indexes without such lists (the loader
            // knows: SearchArgs::flags bit 1 sends the others to the instantiation without it).
            const TailLanes tl = kProbeFirst ? no_tail() : tail_lanes(valid, lane);
            // `fetched`: the lanes whose codes and aux values bl holds -- all of them, or (probe first) the new ones.
            // Returns false when the reference's stage-2 decision cannot be taken from the fetched lanes (probe first only).
            auto estimate = [&](bool fetched) -> bool {
                LaneEst v;
                const float dqp = exact_dist;
                bl.reduce(blk, a.L, qm, lane, v);
                if constexpr (BW == 1) {
                    stage2_est<1>(qp, v, dqp, __builtin_sqrtf(dqp), est, lower, tl);
                } else {
                    // both lower bounds at once, one per lane half (see lower_bounds_split); dqp is the popped vertex's
                    // distance, the same in every lane.  Its usual range, 1e-12 <= dqp < +inf, is one scalar test; the
                    // square root and the one-instruction maxima of the split bounds are only right inside it.  Outside
                    // (the query is a base row, or a norm overflowed) the reference's own two functions run, which
                    // test for the tiny distance themselves -- cold, and the estimate is made in front of the vote.
                    // Both ranges end in the same three arms; `est_of` makes the estimate behind the vote.
                    auto arms = [&](float lo1, float lo2, auto&& est_of) -> bool {
                        // any_survivor (:178-187) ranges over ALL the list's neighbours, estimated before or not
                        if (__builtin_expect((!ST && nn_sz < k) || any64(fetched && valid && lo1 < worst0), 1)) {
                            est = est_of(v);
                            lower = lo2;
                        } else if constexpr (!kProbeFirst) {            // the reference's skipped batch (:201-205)
                            est = FMAX;
                            lower = lo1;
                            skipped2 = true;
                        } else {
                            // Probe first: only the NEW neighbours' codes are here, and none of them survives stage 1.
                            // Whether the reference runs stage 2 then depends on the bounds of neighbours it will skip
                            // anyway (:227) -- which matters only if a new neighbour would ACT on its stage-2 values where
                            // the skipped batch (est = FLT_MAX, lower = stage-1 bound >= worst) makes it do nothing: the two
                            // bounds have different numerators (2 S0 + S1 over 3 against S0) and are not ordered.  No
                            // rerank can happen before such a neighbour's turn without being such an action itself, so the
                            // thresholds of the loop's entry decide: if no new neighbour passes them, both branches leave
                            // the heaps alone and the block's other codes are never needed.  Else the query is handed to
                            // the re-run launch, whose instantiation fetches whole blocks and takes the reference's
                            // decision on the real bounds.  (The stage-1 bounds are loose -- the reference itself never
                            // skips a batch on its own graphs, SURVEY F4 -- so neither happens outside the fixtures that
                            // force it: 0 of 2.65 M expansions on the C2 benchmark.)
                            // (The estimate is computed from a laundered copy of the sum: left recognisable, the compiler
                            // merges this call with the one of the usual branch and hoists both above the ballot, which
                            // measured 15 % slower on the C2 benchmark -- the estimate's division chain then sits in front
                            // of the branch every expansion waits on.)
                            LaneEst w = v;
                            asm volatile("" : "+v"(w.nbit));
                            est = est_of(w);
                            lower = lo2;
                            const bool acts = fetched && !(lo2 >= worst0) && (est < worst0 || est < gamma_q * worst0);
                            if (any64(acts)) return false;
                            undecided2 = true;
                        }
                        return true;
                    };
                    // The static-D forms of the two functions are for the static-D kernels; the runtime-D kernels and
                    // `<2,128,true>` keep the generic square root and the bounds as they were: their register allocation
                    // does not survive the other form (`<2,0,true>` spills a vector register more; `<2,128,true>` takes
                    // 80 registers instead of 78, the ceiling tests/test_steady_loop_resources.py holds it to).
                    constexpr bool kLeanEstimator = SD >= 128 && !(BW == 2 && SD == 128 && kProbeFirst);
                    if constexpr (!kLeanEstimator) {
                        float lo1 = 0.0f, lo2 = 0.0f;
                        const bool tiny = bcast_f32(dqp) < kEpsSmall;
                        if (!tiny) lower_bounds_split<BW>(qp, v, dqp, __builtin_sqrtf(dqp), lane, lo1, lo2, tl);
                        return arms(lo1, lo2, [&](const LaneEst& x) { return stage2_est_only<BW>(qp, x, dqp, tl, tiny); });
                    } else if (__builtin_expect(dqp_in_range(__builtin_amdgcn_readfirstlane(__float_as_uint(dqp))), 1)) {
                        float lo1, lo2;
                        EstShared sh;
                        lower_bounds_split<BW>(qp, v, dqp, sqrt_in_range(dqp), lane, lo1, lo2, tl, sh);
                        return arms(lo1, lo2, [&](const LaneEst& x) { return stage2_est_only<BW>(qp, x, tl, sh); });
                    } else {
                        // (+inf and NaN are in sqrt_in_range's domain; below 1e-12 neither function reads the root)
                        const float sq = sqrt_in_range(dqp);
                        float est_cold, lo2;
                        const float lo1 = stage1_lower<BW>(qp, v, dqp, sq);
                        stage2_est<BW>(qp, v, dqp, sq, est_cold, lo2, tl);
                        return arms(lo1, lo2, [&](const LaneEst&) { return est_cold; });
                    }
                }
                return true;
            };
            // Narrow codes (1- and 2-bit) estimate poorly, so their searches run long, almost always find something new
            // (9 % of the gate workload's expansions are all-seen, 24 % of C2's) and are bound by dependent round trips,
            // not by bandwidth: there the estimator runs BEFORE the probe's result is looked at, under its round trip.
            // The 4-bit kernel keeps the order that skips the arithmetic of all-seen expansions.
            constexpr bool kSpeculate = BW <= 2 && !kProbeFirst;
            if constexpr (kSpeculate) estimate(true);
            CPH_TICKF(4);
#if CPH_PHASE_TIMERS + 0 == 2
            asm volatile("" : "+v"(old_bits));
            CPH_TICKF(5);
#endif

            // ---- estimated set: result of the probe issued above --------------------------------
            bool is_new = active && (old_bits & my_bit) == 0;
            // a vertex whose neighbour list repeats an id: only the first copy is new
            if (!ST && (a.flags & 1u) && any64(is_new)) {    // (steady: the flag was clear where the query changed loops)
                // (graphs written by the reference never repeat an id; the loader sets the
                // flag when one does, and only then is this screen paid for)
#pragma unroll 1   // cold path: rolled, or its 31 lane masks are hoisted and spilled for everyone
                for (int j = 0; j < 31; ++j) {
                    uint32_t oj = __shfl(nid, j);
                    bool nj = __shfl((int)is_new, j) != 0;
                    if (nj && lane > j && lane < 32 && oj == nid) is_new = false;
                }
            }
            const uint32_t new_mask = (uint32_t)(ballot64(is_new) & 0xFFFFFFFFull);
            // mark the new ids (two may share a word) and log them for the un-marking at query end (discovery order =
            // neighbour order) under ONE predicate; a log that would overflow ends the attempt before anything is marked
            const uint32_t n_new = __popc(new_mask);
            const uint32_t my_rank = __builtin_amdgcn_mbcnt_lo(new_mask, 0u);   // set bits below this lane (lanes < 32)
            // The beam must have room for this expansion's pushes (at most one per new id); a query that outgrows its
            // slot is answered by the full-capacity re-run.  The id log only exists to clear the bitmap cheaply: once it
            // is full the query simply stops logging and wipes its whole bitmap at the end (n / 8 bytes -- less than the
            // log it would have needed: a query that discovers more than `cap` ids has touched a good part of the graph).
            if (beam_size + n_new > a.cap) { overflow = true; break; }
            // (two loops: no `wipe` flag is carried from expansion to expansion.  The log's length only grows, and it goes on
            // counting after the log is full, so "full" is a comparison of the length -- here and at query end.)
            bool nolog;
            if constexpr (kRareOffLoop) {
                nolog = log_count + n_new > a.cap;
            } else {
                if (!wipe && log_count + n_new > a.cap) wipe = true;
                nolog = wipe;
            }
            if (is_new) {
                atomicOr(&bm[nid >> 5], my_bit);
                if (!nolog) logi[log_count + my_rank] = nid;
            }
            // Every neighbour already estimated (a quarter to a third of the expansions, most of
            // them late in the search): the reference evaluates the block and then skips all 32
            // neighbours (:227), so nothing it computes is observable -- the FastScan arithmetic,
            // more than half of an expansion's vector instructions, is not issued at all.
            if (new_mask == 0) {
                ++st_allseen;
                continue;
            }
            if constexpr (kProbeFirst) {
                const bool fetch = ((new_mask >> (lane & 31)) & 1u) != 0u;       // both lane halves of a new neighbour
                // The codes and aux values are loaded behind the probe by the lanes of the new neighbours only (`fetch`
                // below).  The other lanes' registers are left UNDEFINED -- whatever the previous expansion left there --
                // instead of being zeroed (4 kCPL + 4 v_mov per expansion with a new neighbour).  Such a lane computes
                // est / lower from garbage (there are no floating-point traps on this path, and no address is formed
                // from these values), and none of it is observable: every reader is masked by a set of lanes that
                // `fetch` contains -- fetch = new_mask's bit of (lane & 31), is_new = that bit in the lower lane half:
                //   estimate(): any64(fetched && valid && lo1 < worst0)              -> fetched (= fetch)
                //   estimate(): acts = fetched && ...                                -> fetched
                //   cand = is_new && ...  (cand_mask, s_list, the speculative exact L2) -> is_new
                //   lane-parallel pushes: p = is_new && ...  (pm, the parent check under chk = p && .., the append) -> p
                //   serial replay: m = new_mask [& ballot(!(lower >= worst0))], v_readlane of est / lower at the set
                //   bits of m only                                                   -> new_mask
                //   replay of the lane-parallel pushes: v_readlane at the set bits of pm -> p
                // (the same readers in both copies of the loop: the steady one only drops the warm-up arms of cand and m;
                // its own lane-parallel arm builds the entry in every lane and reads it, like the general one, under p)
                bl.leave_undefined();
                if (fetch) bl.issue_static(blk, lane);
                if (__builtin_expect(!estimate(fetch), 0)) { overflow = true; stage2_redo = true; break; }
            } else if constexpr (!kSpeculate) {
                estimate(true);
            }
            if (skipped2) st_skip++;
            if (undecided2) st_undecided++;

            CPH_TICK(2);
            const bool warmup = !ST && nn_sz < k;  // (:210; read at the head: an expansion whose replay fills the heap ends as a warm-up one)
            bool cand = is_new && (warmup || (!(lower >= worst0) && est < worst0));
            const uint32_t cand_mask = (uint32_t)(ballot64(cand) & 0xFFFFFFFFull);

            if constexpr (!kDerivedCounters) st_new += n_new;
            CPH_TICK(3);

            // ---- speculative exact L2 of the candidates, 8 per pass (rare: ~0.15 per expansion) --
            // Filtered: the allowed bits of the new neighbours -- the only ones the serial replay below can push into the
            // result heap -- as one lane-parallel load, issued ahead of the exact-L2 loads and turned into a mask behind
            // them.  The replay is taken exactly when cand_mask != 0 (in the warm-up cand_mask == new_mask != 0), so the mask
            // is ready wherever it is read; the lane-parallel path (no candidate) never touches the result heap.
            uint32_t allow_mask = 0;
            if (cand_mask) {
                uint32_t allow_w = 0;
                if constexpr (FTAB) allow_w = allow_q[is_new ? nid >> 5 : 0u];
                else if constexpr (FILT) allow_w = CPH_COLD(allow)[is_new ? nid >> 5 : 0u];
                if (cand) s_list[__builtin_amdgcn_mbcnt_lo(cand_mask, 0u)] = (uint8_t)lane;
                __syncthreads();
                const uint32_t n_cand = __popc(cand_mask);
                const int g = lane >> 3;
                for (uint32_t base = 0; base < n_cand; base += 8) {
                    const bool have = base + g < n_cand;
                    const uint32_t idx = have ? s_list[base + g] : 0;
                    const uint32_t cid_l = (uint32_t)__shfl((int)nid, (int)idx);
                    const uint32_t cid = have ? cid_l : cur_id;
                    const float cnorm = a.norm_sq[cid];   // issued with the vector loads, not after them
                    float dot = group_dot8_lo(qv, a.raw + (size_t)cid * D, D, lane & 7);
                    float ex = exact_from_dot(qnorm, cnorm, dot);
                    asm volatile("" ::"v"(ex));   // keeps the norm load out of the branch below
                    if (have && (lane & 7) == 0) s_exact[idx] = ex;
                }
                // (two loops: added to the wave's total in LDS where it happens, not carried in a register)
                if constexpr (kRareOffLoop) { if (lane == 0) s_tot[kStatExact] += n_cand; }
                else st_exact += n_cand;
                __syncthreads();
                if constexpr (FILT) allow_mask = (uint32_t)(ballot64(is_new && ((allow_w >> (nid & 31u)) & 1u) != 0u) & 0xFFFFFFFFull);
            }
            CPH_TICK(4);
            CPH_TICKF(6);

            // ---- serial replay of the neighbour loop (:218-273).  The loop runs on lane 0 (heap
            // state lives there) but `i` comes from the wave-uniform ballot mask, so neighbour i's
            // est / lower / id are read straight out of lane i's registers with v_readlane ------
            if (!warmup && cand_mask == 0) {
                // No neighbour of this vertex is reranked, so the result heap, its threshold and
                // gamma_q stay what they were at loop entry: every decision of the serial loop is
                // `lower < worst0 <= est < gamma_q * worst0` and can be taken by all lanes at once;
                // only the beam pushes themselves keep neighbour order.
                const float dabs0 = gamma_q * worst0;
                const bool p = is_new && !(lower >= worst0) && est < dabs0;
                uint32_t pm = (uint32_t)(ballot64(p) & 0xFFFFFFFFull);
                // std::push_heap of each in neighbour order.  Usual case: every new entry is no
                // better than the parent of the leaf it lands on, so nothing moves and the pushes
                // are independent appends -- each lane checks its own parent and writes its own leaf.
                const uint32_t np = __popc(pm);
                bool appended = false;      // (general copy only: the steady arm clears `pm` instead)
                if constexpr (ST) {
                    // Steady copy: the same decisions as the general arm below (keep the two in step), shaped for the
                    // compiler's control-flow pass (the loop holds divergent branches, so its uniform branches are rebuilt
                    // with it: a bool that is live across a join -- `appended`, `in_lds` -- and every && of two uniform
                    // tests comes back as a lane mask, s_cselect_b64 -1,0 / s_and_b64 vcc,exec / s_cbranch_vcc, plus
                    // copies on the latch).  Here every uniform test is ONE scalar compare with its own branch, no flag
                    // crosses a join -- the appended pushes leave the mask, and the serial loop below runs on what is
                    // left of it --, and the beam in LDS, the usual case, has an arm of its own.
                    // profiles/steady_tail.md: 43 scalar instructions fewer on the usual expansion.
                    CPH_CENSUS(7);
                    const uint4 ent = make_uint4(__float_as_uint(est), __float_as_uint(lower), nid, 0u);
                    if (np - 1u <= beam_size) {               // np != 0 && np <= beam_size + 1, as one unsigned compare
                        __builtin_amdgcn_wave_barrier();      // (no instruction: keeps the two compares two branches)
                        if (beam_size + np <= kBeamLds) {     // in LDS (implies !(np == 1 && beam_size >= kBeamLds))
                            const uint32_t pos = beam_size + __builtin_amdgcn_mbcnt_lo(pm, 0u);
                            // every lane reads a parent (lanes without a push: the root) and is masked afterwards
                            const bool chk = p && pos > 0;
                            const bool stay = !(heap.lds_key(chk ? (pos - 1) >> 1 : 0u) > est) || !chk;
                            if (all64(stay)) {
                                CPH_CENSUS(0);
                                if (p) heap.lds_put(pos, ent);
                                beam_size += np;
                                st_push += np;
                                pm = 0;
                            } else {
                                CPH_CENSUS(3);
                            }
                        // (a single push onto a spilled beam goes straight to the push routine: the parent check of the
                        // append path would be a dependent round trip of its own in front of the one the routine makes anyway)
#ifdef CPH_NO_SKIP_APPEND
                        } else {
#else
                        } else if (np != 1) {
#endif
                            const uint32_t pos = beam_size + __builtin_amdgcn_mbcnt_lo(pm, 0u);
                            bool stay = true;
                            if (p && pos > 0) stay = !(heap.raw_key((pos - 1) >> 1) > est);
                            if (all64(stay)) {
                                CPH_CENSUS(1);
#ifdef CPH_TRAFFIC_STATS
                                trf[3]++;
#endif
                                if (p) heap.put(pos, ent);
                                beam_size += np;
                                st_push += np;
                                pm = 0;
                            } else {
                                CPH_CENSUS(3);
                            }
#ifndef CPH_NO_SKIP_APPEND
                        } else {
                            CPH_CENSUS(2);
#endif
                        }
                    } else if (np == 0) {
                        CPH_CENSUS(4);
                    } else {
                        CPH_CENSUS(5);
                    }
                } else
                // General copy and every one-loop instantiation (the steady arm above takes the same decisions).
                // (a single push onto a spilled beam goes straight to the push routine: the parent check of the append path
                // would be a dependent round trip of its own in front of the one the routine makes anyway)
#ifdef CPH_NO_SKIP_APPEND
                if (np != 0 && np <= beam_size + 1) {
#else
                if (np != 0 && np <= beam_size + 1 && !(np == 1 && beam_size >= kBeamLds)) {
#endif
                    const uint32_t pos = beam_size + __builtin_amdgcn_mbcnt_lo(pm, 0u);
                    const bool in_lds = beam_size + np <= kBeamLds;   // wave-uniform: the usual case keeps its ds_* accesses
                    bool stay = true;
                    if (in_lds) {
                        // every lane reads a parent (lanes without a push: the root) and is masked afterwards
                        const bool chk = p && pos > 0;
                        stay = !(heap.lds_key(chk ? (pos - 1) >> 1 : 0u) > est) || !chk;
                    } else if (p && pos > 0) {
                        stay = !(heap.raw_key((pos - 1) >> 1) > est);
                    }
                    if (all64(stay)) {
#ifdef CPH_TRAFFIC_STATS
                        if (!in_lds) trf[3]++;
#endif
                        const uint4 ent = make_uint4(__float_as_uint(est), __float_as_uint(lower), nid, 0u);
                        if (p) { if (in_lds) heap.lds_put(pos, ent); else heap.put(pos, ent); }
                        beam_size += np;
                        st_push += np;
                        appended = true;
                    }
                }
                if (ST || !appended) {
                    while (pm) {
                        const int i = __ffs((int)pm) - 1;
                        pm &= pm - 1;
                        const uint32_t id_i = (uint32_t)__builtin_amdgcn_readlane((int)nid, i);
                        const uint32_t e_i = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(est), i);
                        const uint32_t lo_i = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(lower), i);
#ifdef CPH_TRAFFIC_STATS
                        if (beam_size >= kBeamLds) trf[2]++;
#endif
                        if (beam_size < kBeamLds) heap_push_wave(heap, beam_size, make_uint4(e_i, lo_i, id_i, 0u), lane);
                        else beam_push_hybrid(heap, beam_size, make_uint4(e_i, lo_i, id_i, 0u), lane);
                        ++beam_size;
                        ++st_push;
                    }
                }
            } else {
                CPH_CENSUS(6);
                // past the warm-up the threshold only falls: a lower bound that fails it at loop
                // entry fails it at its turn too (:241), so those neighbours are dropped here
                uint32_t m = warmup ? new_mask
                                    : new_mask & (uint32_t)(ballot64(!(lower >= worst0)) & 0xFFFFFFFFull);
                // Every quantity of the reference's loop body is wave-uniform here (neighbour i's values come out
                // of lane i with v_readlane, the heaps live in LDS), so the whole wave walks the loop together and
                // the heap operations are the wave-parallel ones: a rerank costs two LDS round trips per heap
                // operation instead of one dependent round trip per heap level on lane 0.
                while (m) {
                    const int i = __ffs((int)m) - 1;
                    m &= m - 1;
                    const uint32_t id_i = (uint32_t)__builtin_amdgcn_readlane((int)nid, i);
                    const float e = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(est), i));
                    const float lo_i = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(lower), i));
                    const float worst = bcast_f32(nnw.lds_key(0));   // FLT_MAX while the heap is empty
                    const float dabs = (ST || nn_size >= k) ? gamma_q * worst : FMAX;
                    // 1 = rerank (result-heap push), 4 = ... and feed the gamma adaptation, 2 = DABS enqueue on the estimate
                    uint32_t act = 0;
                    if (warmup) act = 1;
                    else if (!(lo_i >= worst)) act = (e < worst) ? 5u : ((e < dabs) ? 2u : 0u);
                    act = bcast_u32(act);
                    float key = e, lo = lo_i;
                    bool push = (act & 2u) != 0;
                    if (act & 1u) {
                        const float ex = bcast_f32(s_exact[i]);
                        if (!FILT || ((allow_mask >> i) & 1u) != 0u) nn_push_wave<ST>(nnw, nn, nn_size, k, id_i, ex, worst, lane);
                        if (ex < dabs) { push = true; key = ex; if (warmup) lo = ex; }
                        if ((act & 4u) && ex > kEpsSmall) {
                            // gamma adaptation (:255-267), fused as the reference compiles it; fp64 on one lane
                            ++ratio_count;
                            if (lane == 0) {
                                double r = (double)(e / ex);
                                const double rs = s_ratio[0] + r;
                                const double rq = fma(r, r, s_ratio[1]);
                                s_ratio[0] = rs;
                                s_ratio[1] = rq;
                                if (ratio_count >= a.sc.gamma_warmup) {
                                    double cnt = (double)ratio_count;
                                    double mean = rs / cnt;
                                    double var = fma(-mean, mean, rq / cnt);
                                    double sd = sqrt(var < 0.0 ? 0.0 : var);
                                    float gq = gamma * (float)fma((double)a.sc.gamma_beta, sd, 1.0);
                                    gamma_q = (gq < gamma) ? gamma
                                                           : ((a.sc.gamma_max < gq) ? a.sc.gamma_max : gq);
                                }
                            }
                            gamma_q = bcast_f32(gamma_q);
                        }
                    }
                    if (any64(push)) {             // (every lane agrees)
                        const uint4 ent = beam_pack(BeamEntry{key, lo, id_i});
#ifdef CPH_TRAFFIC_STATS
                        if (beam_size >= kBeamLds) trf[2]++;
#endif
                        if (beam_size < kBeamLds) heap_push_wave(heap, beam_size, ent, lane);
                        else beam_push_hybrid(heap, beam_size, ent, lane);
                        ++beam_size;
                        ++st_push;
                    }
                }
                CPH_TICK(4);      // (timer builds: the serial replay is booked with the speculative rerank)
            }
            CPH_TICK(5);
            log_count += n_new;
            // one wave per workgroup: LDS accesses of a wave execute in program order, so only the
            // compiler needs a fence here -- an s_barrier would also drain the prefetch (vmcnt)
            __builtin_amdgcn_wave_barrier();
            CPH_TICK(6);
            CPH_TICKF(7);
        }
