// CTC prefix beam search with an optional character n-gram LM: the search side of the reference's decode_with_lm
// (src/decoder.py:11-109, src/models/cnnlstm.py:298-475), with a character n-gram in ARPA form standing in for the eesen WFST.
//
// One workgroup of 256 threads per line; workgroups never talk to each other (no spins, no grid barrier).  Per frame t < lens[b]:
//   1. row log-softmax of the raw logits in fp32 (one column per thread, V <= 256), then the SYMBOL CLASSES: a class is a
//      canonical column c (canon[c] == c); its log-probability is the logsumexp of its member columns (canon[v] == c), so
//      English 'u002d' at 73 and 91 is one symbol, as in the greedy collapse.  Emitted labels are canonical indices.
//   2. per beam j: the "stay" probabilities (blank, or the repeat of the last class), and the MERGE of the extension that
//      re-creates prefix j from a beam k holding j's parent prefix.  Identity of prefixes is exact: a 64-bit rolling hash plus
//      the length filter, and every hash match is confirmed by walking both node chains in the pool until they meet at one node
//      (same node => same rest of the prefix) or a class differs.  A prefix that left the beam and came back under a new node id
//      while its child stayed is therefore still found.
//   3. candidate scores  logsumexp(p_b, p_nb) + lm_weight * LM + insertion_bonus * len  for the K*V candidates (slot k*V + 0 is
//      beam k's stay, slot k*V + c the extension by class c), into LDS.
//   4. the top K under a TOTAL order: score, then the slot id k*V + c (k = the parent's rank).  Radix select over the fp32 bits of
//      the score (4 passes of 8 bits, histograms in LDS), and where several candidates share the K-th score, two more passes over
//      the ids of those.  Only integer LDS atomics; every float is computed by a fixed thread in a fixed order, so the output is
//      bit-identical from run to run and independent of thread timing.  The kept candidates are ranked by counting (K^2 compares)
//      and become the new beams in rank order.
//   5. each new prefix gets node t*K + rank in the pool: (parent node, class), no allocation counter.
// At the end of the line alpha * ln P(</s> | state) is added, the beams are ranked once more and the top `nbest` are backtracked.
//
// Why stored scores and radix select: the K*V candidate SCORES alone fit in LDS (K = 128, V = 256: 128 KiB; the slot id is the
// position, so no (score, id) pairs are stored), and four passes over LDS are cheaper than recomputing the candidates (with
// their LM loads) per pass or merging K sorted per-beam lists.  Static LDS (two beam-state buffers, class log-probs, histogram,
// selection) is about 20 KiB, so the worst case takes ~148 KiB of the 160 KiB per CU: one line per CU, which is what the
// problem has (B lines << 256 CUs).
//
// LM: backoff-resolved dense tables over S states, lm_logp[S][V] (natural log), lm_next[S][V], lm_eos[S]; a candidate costs one
// load of each, coalesced over c.  State indices read from lm_next outside [0, S) fall back to lm_start (never an out-of-range load).
// prune_logp: classes whose frame log-prob is below it are not extended (-inf: off, the exact search).
//
// Steps 1, 2 (the merge lookup), 4 and the backtrack are the device functions of ctc_beam_common.h, shared with the word search
// (ctc_word_beam.hip); this file holds the character LM's candidate scoring and beam state.
#include "ctc_beam_common.h"

namespace {

using namespace ctcbeam;

struct BeamBuf {
    float pb[KMAX], pnb[KMAX], acc[KMAX];
    int last[KMAX], len[KMAX], lms[KMAX], node[KMAX];
    unsigned long long hash[KMAX], phash[KMAX];
};

__global__ __launch_bounds__(BT) void ctc_beam_kernel(const float* __restrict__ logits, const int32_t* __restrict__ lens, int T, int B,
                                                      int V, const int32_t* __restrict__ canon, int K, int nbest,
                                                      const float* __restrict__ lm_logp, const int32_t* __restrict__ lm_next,
                                                      const float* __restrict__ lm_eos, int S, int lm_start, float alpha, float beta,
                                                      float prune, int32_t* __restrict__ out_labels, int32_t* __restrict__ out_lens,
                                                      float* __restrict__ out_scores, int2* __restrict__ pool_all) {
    extern __shared__ float s_score[];                 // [K*V]
    __shared__ BeamBuf s_beam[2];
    __shared__ Frame s_f;
    __shared__ Select s_sel;
    __shared__ float s_spb[KMAX], s_spnb[KMAX], s_fin[KMAX];
    __shared__ int s_merge[KMAX];

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const bool has_lm = lm_logp != nullptr;
    const int start = has_lm ? lm_start : 0;
    const int len_b = min(max(lens[b], 0), T);
    int2* pool = pool_all + (long)b * T * K;

    init_classes(canon, V, s_f);
    if (tid == 0) {
        BeamBuf& B0 = s_beam[0];
        B0.pb[0] = 0.f; B0.pnb[0] = NEG_INF; B0.acc[0] = 0.f; B0.last[0] = -1; B0.len[0] = 0; B0.lms[0] = start;
        B0.node[0] = -1; B0.hash[0] = HASH_ROOT; B0.phash[0] = 0;
    }
    int cur = 0, nb = 1;
    __syncthreads();

    for (int t = 0; t < len_b; ++t) {
        const BeamBuf& C = s_beam[cur];
        BeamBuf& N = s_beam[cur ^ 1];
        // 1. log-softmax of the row, class log-probs
        frame_logprobs(logits + ((long)t * B + b) * V, V, prune, s_f);

        // 2. stay probabilities and the merge of the extension that re-creates beam j from its parent prefix
        if (tid < nb) {
            const int j = tid;
            const int lj = C.len[j], cj = C.last[j];
            const int mk = find_merge(j, nb, C.len, C.last, C.node, C.hash, C.phash, s_f.xp, pool, T * K);
            s_merge[j] = mk;
            const float pbj = C.pb[j], pnbj = C.pnb[j];
            float spnb = lj > 0 ? pnbj + s_f.lp[cj] : NEG_INF;
            if (mk >= 0) {
                const float base = (cj == C.last[mk]) ? C.pb[mk] : lse2(C.pb[mk], C.pnb[mk]);
                spnb = lse2(spnb, base + s_f.xp[cj]);
            }
            s_spb[j] = lse2(pbj, pnbj) + s_f.lp[0];
            s_spnb[j] = spnb;
        }
        __syncthreads();

        // 3. candidate scores
        const int ncand = nb * V;
        for (int i = tid; i < ncand; i += BT) {
            const int k = i / V, c = i - k * V;
            float sc;
            if (c == 0) {
                const float ac = lse2(s_spb[k], s_spnb[k]);
                sc = ac + (has_lm && alpha != 0.f ? alpha * C.acc[k] : 0.f) + beta * (float)C.len[k];
            } else {
                const float xp = s_f.xp[c];
                if (xp == NEG_INF) {
                    sc = NEG_INF;
                } else {
                    const float pnb = ((c == C.last[k]) ? C.pb[k] : lse2(C.pb[k], C.pnb[k])) + xp;
                    const float lmv = has_lm ? C.acc[k] + lm_logp[(long)C.lms[k] * V + c] : 0.f;
                    sc = pnb + (has_lm && alpha != 0.f ? alpha * lmv : 0.f) + beta * (float)(C.len[k] + 1);
                }
            }
            s_score[i] = sc;
        }
        __syncthreads();
        if (tid < nb && s_merge[tid] >= 0) s_score[s_merge[tid] * V + C.last[tid]] = NEG_INF;
        __syncthreads();

        // 4. top K under (score desc, id asc)
        const int nsel = top_k(s_score, ncand, K, s_sel);

        // 5. the new beams, in rank order
        if (tid < nsel) {
            const int q = tid, id = s_sel.order[q];
            const int k = id / V, c = id - k * V;
            if (c == 0) {
                N.pb[q] = s_spb[k]; N.pnb[q] = s_spnb[k]; N.acc[q] = C.acc[k]; N.last[q] = C.last[k]; N.len[q] = C.len[k];
                N.lms[q] = C.lms[k]; N.node[q] = C.node[k]; N.hash[q] = C.hash[k]; N.phash[q] = C.phash[k];
            } else {
                const int node = t * K + q;
                N.pb[q] = NEG_INF;
                N.pnb[q] = ((c == C.last[k]) ? C.pb[k] : lse2(C.pb[k], C.pnb[k])) + s_f.xp[c];
                if (has_lm) {
                    const long e = (long)C.lms[k] * V + c;
                    const int ns = lm_next[e];
                    N.acc[q] = C.acc[k] + lm_logp[e];
                    N.lms[q] = (ns >= 0 && ns < S) ? ns : start;
                } else {
                    N.acc[q] = 0.f;
                    N.lms[q] = 0;
                }
                N.last[q] = c; N.len[q] = C.len[k] + 1; N.node[q] = node;
                N.hash[q] = hash_push(C.hash[k], c); N.phash[q] = C.hash[k];
                pool[node] = make_int2(C.node[k], c);
            }
        }
        nb = nsel;
        cur ^= 1;
        __syncthreads();
    }

    // end of line: + alpha * ln P(</s> | state), final ranking (ties: the rank at the last frame), backtrack the top nbest
    const BeamBuf& C = s_beam[cur];
    if (tid < nb) {
        const float lmt = has_lm ? C.acc[tid] + lm_eos[C.lms[tid]] : 0.f;
        s_spb[tid] = lse2(C.pb[tid], C.pnb[tid]);
        s_spnb[tid] = lmt;
        s_fin[tid] = s_spb[tid] + (has_lm && alpha != 0.f ? alpha * lmt : 0.f) + beta * (float)C.len[tid];
    }
    __syncthreads();
    rank_final(s_fin, nb, s_sel.order);
    if (tid < nbest) {
        const int q = tid;
        const int j = q < nb ? s_sel.order[q] : 0;
        write_hyp(b, q, nbest, T, q < nb, C.len[j], C.node[j], s_fin[j], s_spb[j], s_spnb[j], pool, T * K, out_labels, out_lens,
                  out_scores);
    }
}

}  // namespace

extern "C" size_t vocr_ctc_beam_workspace_bytes(int t, int b, int v, int beam, int nbest) {
    if (t <= 0 || b <= 0 || v <= 0 || v > VMAX || beam < 1 || beam > KMAX || nbest < 1 || nbest > beam) return 0;
    return (size_t)t * b * beam * sizeof(int2);
}

extern "C" int vocr_ctc_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam,
                                    int nbest, const float* lm_logp, const int32_t* lm_next, const float* lm_eos, int lm_states,
                                    int lm_start, float lm_weight, float insertion_bonus, float prune_logp, int32_t* out_labels,
                                    int32_t* out_lens, float* out_scores, void* workspace, size_t workspace_bytes, void* stream) {
    VOCR_CHECK_ARG(logits && lens && out_labels && out_lens && out_scores && workspace, "vocr_ctc_beam_search: null pointer");
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 0 && v <= VMAX, "vocr_ctc_beam_search: need t > 0, b > 0, 1 <= v <= %d (t=%d b=%d v=%d)", VMAX,
                   t, b, v);
    VOCR_CHECK_ARG(beam >= 1 && beam <= KMAX, "vocr_ctc_beam_search: need 1 <= beam <= %d (beam=%d)", KMAX, beam);
    VOCR_CHECK_ARG(nbest >= 1 && nbest <= beam, "vocr_ctc_beam_search: need 1 <= nbest <= beam (nbest=%d beam=%d)", nbest, beam);
    VOCR_CHECK_ARG((long)t * b * beam < (1L << 31) && (long)t * beam < (1L << 30), "vocr_ctc_beam_search: t*b*beam too large");
    const bool any_lm = lm_logp || lm_next || lm_eos;
    VOCR_CHECK_ARG(!any_lm || (lm_logp && lm_next && lm_eos), "vocr_ctc_beam_search: lm_logp, lm_next and lm_eos go together");
    VOCR_CHECK_ARG(!any_lm || (lm_states >= 1 && lm_start >= 0 && lm_start < lm_states),
                   "vocr_ctc_beam_search: need 0 <= lm_start < lm_states (lm_start=%d lm_states=%d)", lm_start, lm_states);
    VOCR_CHECK_ARG(__builtin_isfinite(lm_weight) && __builtin_isfinite(insertion_bonus) && !__builtin_isnan(prune_logp),
                   "vocr_ctc_beam_search: lm_weight and insertion_bonus must be finite, prune_logp not NaN");
    const size_t need = vocr_ctc_beam_workspace_bytes(t, b, v, beam, nbest);
    VOCR_CHECK_ARG(workspace_bytes >= need, "vocr_ctc_beam_search: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_beam_kernel};
    if (vocr_allow_dynamic_lds(big, 1, KMAX * VMAX * (int)sizeof(float), &lds_set, "vocr_ctc_beam_search") != VOCR_OK) return VOCR_ELAUNCH;
    const size_t lds = (size_t)beam * v * sizeof(float);
    ctc_beam_kernel<<<b, BT, lds, (hipStream_t)stream>>>(logits, lens, t, b, v, canon, beam, nbest, any_lm ? lm_logp : nullptr, lm_next,
                                                         lm_eos, any_lm ? lm_states : 1, any_lm ? lm_start : 0, lm_weight,
                                                         insertion_bonus, prune_logp, out_labels, out_lens, out_scores,
                                                         (int2*)workspace);
    VOCR_CHECK_LAUNCH("vocr_ctc_beam_search");
    return VOCR_OK;
}
