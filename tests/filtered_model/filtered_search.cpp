// TEST INFRASTRUCTURE — the model of the filtered search the GPU tests compare against.
//
// The oracle's search (oracle/cph_oracle.cpp: search_one, a restatement of the reference's
// rabitq_search.hpp:60-277) with one change: a vertex enters the result heap only if its id is allowed,
// i.e. `nn_push(r)` becomes `if (allowed(r.id)) nn_push(r)` at its three call sites (the popped vertex, the
// warm-up neighbours, the reranked neighbours).  Everything else -- estimates, reranks, beam pushes, the
// gamma statistics, the termination tests on nn.size() / nn_worst() -- is the oracle's, line for line.
// Built at test time with the oracle's own flags (tests/filtered_model_lib.py).
#include "../../oracle/cph_oracle.cpp"

namespace {

// allow = bit (id & 31) of allow[id >> 5]; null: every id allowed (the unfiltered search)
int search_one_filtered(const Index& ix, const float* query /*dim*/, size_t k, const uint32_t* allow,
                        std::vector<Result>& out, Counters* ctr) {
    const size_t D = ix.D, bw = ix.bw;
    const Layout& L = ix.L;
    std::vector<float> q(D, 0.0f);
    std::memcpy(q.data(), query, ix.dim * sizeof(float));
    QueryCode qc;
    encode_query(*ix.rot, q.data(), qc, nullptr);
    QParams qp{qc.A, qc.B, qc.C, ix.affine_a, ix.affine_b, ix.ip_qo_floor, ix.slack_levels[0]};
    if (k < 1) k = 1;
    float gamma = ix.search_gamma;

    uint32_t ep = ix.entry;
    if (ix.max_level > 0)
        for (int level = ix.max_level; level >= 1; --level) ep = greedy_layer(ix, q.data(), ep, level);
    if (ep == kInvalid || ep >= ix.n) return -1;

    std::vector<uint8_t> estimated(ix.n, 0), visited(ix.n, 0);
    std::vector<BeamEntry> beam;
    std::vector<Result> nn;
    nn.reserve(k + 1);
    auto allowed = [&](uint32_t id) { return allow == nullptr || ((allow[id >> 5] >> (id & 31)) & 1u) != 0u; };
    auto nn_worst = [&]() { return nn.empty() ? std::numeric_limits<float>::max() : nn[0].dist; };
    auto nn_push = [&](Result r) {
        if (!allowed(r.id)) return;   // the only change against search_one
        if (nn.size() < k) { nn.push_back(r); heap_push(nn.data(), nn.size(), result_before); }
        else if (r.dist < nn[0].dist) {
            heap_pop(nn.data(), nn.size(), result_before);
            nn.back() = r;
            heap_push(nn.data(), nn.size(), result_before);
        }
    };
    auto beam_push = [&](BeamEntry e) {
        beam.push_back(e); heap_push(beam.data(), beam.size(), beam_before);
        if (ctr) { ctr->beam_push++; if (beam.size() > ctr->beam_max) ctr->beam_max = beam.size(); }
    };

    float gamma_q = gamma;
    double ratio_sum = 0.0, ratio_sq_sum = 0.0;
    uint64_t ratio_count = 0;
    float qnorm = dot8(D, q.data(), q.data());
    auto exact_l2 = [&](uint32_t id) {
        if (ctr) ctr->exact_l2++;
        float v = (qnorm + ix.norm_sq[id]) - 2.0f * dot8(D, q.data(), ix.vec(id));
        return v > 0.0f ? v : 0.0f;
    };

    beam_push({exact_l2(ep), 0.0f, ep});
    estimated[ep] = 1;
    uint32_t fs[32], msb[32];
    float est[32], lower[32];
    int slack_batch = 0;

    while (!beam.empty()) {
        BeamEntry cur{};
        bool found = false;
        while (!beam.empty()) {
            cur = beam[0];
            heap_pop(beam.data(), beam.size(), beam_before);
            beam.pop_back();
            if (visited[cur.id]) continue;
            found = true;
            break;
        }
        if (!found) break;
        if (nn.size() >= k && cur.est >= gamma_q * nn_worst()) { if (ctr) ctr->gamma_breaks++; break; }
        if (nn.size() >= k && cur.lower > nn_worst()) { if (ctr) ctr->lb_pruned_pops++; continue; }
        visited[cur.id] = 1;
        float exact_dist = exact_l2(cur.id);
        nn_push({cur.id, exact_dist});
        if (ctr) ctr->expansions++;

        const uint8_t* nb = ix.nb(cur.id);
        uint32_t count = rd<uint32_t>(nb + L.count);
        if (count == 0) continue;
        float dqp = exact_dist;
        if (ix.num_slack_levels > 0) {
            int li = std::min(slack_batch, ix.num_slack_levels - 1);
            qp.slack = ix.slack_levels[li];
            ++slack_batch;
        }
        const float* nop = (const float*)(nb + L.nop);
        const float* ipqo = (const float*)(nb + L.ip_qo);
        const float* ipcp = (const float*)(nb + L.ip_cp);
        const uint16_t* pop = (const uint16_t*)(nb + L.pop);
        const uint32_t* ids = (const uint32_t*)(nb + L.ids);
        int bc = (int)std::min<uint32_t>(32, count);
        if (bw == 1) {
            plane_sums(D, qc.lut.data(), nb + L.codes, fs);
            convert_1bit(qp, fs, nop, ipqo, ipcp, pop, bc, dqp, est, lower);
        } else {
            const uint16_t* wpop = (const uint16_t*)(nb + L.wpop);
            msb_sums(D, bw, qc.lut.data(), nb + L.codes, msb);
            convert_msb(bw, qp, msb, nop, ipqo, ipcp, pop, bc, dqp, lower);
            float thr = nn_worst();
            bool any = nn.size() < k;
            if (!any) for (int j = 0; j < bc; ++j) if (lower[j] < thr) { any = true; break; }
            if (any) {
                nbit_sums(D, bw, qc.lut.data(), nb + L.codes, fs, msb);
                convert_nbit(bw, qp, fs, msb, nop, ipqo, ipcp, pop, wpop, bc, dqp, est, lower);
            } else {
                if (ctr) ctr->stage2_skipped++;
                for (int j = 0; j < bc; ++j) est[j] = std::numeric_limits<float>::max();
            }
        }
        bool warmup = nn.size() < k;
        for (uint32_t i = 0; i < count; ++i) {
            uint32_t nid = ids[i];
            if (ctr) ctr->nbr_seen++;
            if (estimated[nid]) continue;
            estimated[nid] = 1;
            if (ctr) ctr->nbr_new++;
            float dabs = (nn.size() >= k) ? gamma_q * nn_worst() : std::numeric_limits<float>::max();
            if (warmup) {
                float ex = exact_l2(nid);
                nn_push({nid, ex});
                if (ex < dabs) beam_push({ex, ex, nid});
                continue;
            }
            float e = est[i], lo = lower[i];
            if (nn.size() >= k && lo >= nn_worst()) continue;
            if (e < nn_worst()) {
                float ex = exact_l2(nid);
                nn_push({nid, ex});
                if (ex < dabs) beam_push({ex, lo, nid});
                if (ex > kEpsSmall) {
                    double r = (double)(e / ex);
                    ratio_sum += r;
                    ratio_sq_sum = std::fma(r, r, ratio_sq_sum);
                    ++ratio_count;
                    if (ratio_count >= ix.gamma_warmup) {
                        double nn_ = (double)ratio_count;
                        double mean = ratio_sum / nn_;
                        double var = std::fma(-mean, mean, ratio_sq_sum / nn_);
                        double sd = std::sqrt(var < 0.0 ? 0.0 : var);
                        float g = gamma * (float)std::fma((double)ix.gamma_beta, sd, 1.0);
                        gamma_q = (g < gamma) ? gamma : ((ix.gamma_max < g) ? ix.gamma_max : g);
                    }
                }
            } else if (e < dabs) {
                beam_push({e, lo, nid});
            }
        }
    }
    heap_sort(nn.data(), nn.size(), result_before);
    out = nn;
    return 0;
}

}  // namespace

extern "C" {

// orc_search_batch with an allowed-id bitmap (allow_words: bit id & 31 of word id >> 5; null = all allowed):
// ids/dists [n][k] padded with -1 / FLT_MAX, counts[i] = real results, counters (optional) = the same 9 u64 per query.
int flt_search_batch(void* h, const float* queries, long n, long k, const uint32_t* allow_words, int64_t* ids,
                     float* dists, int32_t* counts, uint64_t* counters, int nthreads) {
    Index* ix = static_cast<Index*>(h);
    int rc = 0;
    if (nthreads <= 0) nthreads = omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 4) num_threads(nthreads)
    for (long i = 0; i < n; ++i) {
        std::vector<Result> res;
        Counters c{};
        int r = search_one_filtered(*ix, queries + i * ix->dim, (size_t)k, allow_words, res, counters ? &c : nullptr);
        if (r != 0) {
#pragma omp atomic write
            rc = r;
        }
        long j = 0;
        for (; j < (long)res.size() && j < k; ++j) {
            ids[i * k + j] = res[j].id; dists[i * k + j] = res[j].dist;
        }
        if (counts) counts[i] = (int32_t)res.size();
        for (; j < k; ++j) { ids[i * k + j] = -1; dists[i * k + j] = std::numeric_limits<float>::max(); }
        if (counters) std::memcpy(counters + i * 9, &c, sizeof(c));
    }
    return rc;
}

}  // extern "C"
