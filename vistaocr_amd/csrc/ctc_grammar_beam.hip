// Grammar-constrained CTC prefix beam search: the most probable labellings that a deterministic finite automaton ACCEPTS, with the
// optional character n-gram of vocr_ctc_beam_search alongside.  vocr_ctc_grammar_scores says how probable it is that a line belongs
// to a regular language and returns the best single PATH; this search sums the paths of each labelling, as the two other searches
// do, and keeps only prefixes the automaton can still complete.
//
// The kernel is ctc_beam.hip's: one workgroup of 256 threads per line, the same class log-probabilities, stay / extend candidates,
// exact merge, radix top-K, node pool, final ranking and backtrack (ctc_beam_common.h), the same LM tables and score formula.  The
// candidate arithmetic is written as the same expressions, so that under the one-state automaton that accepts everything the
// search takes the decisions of vocr_ctc_beam_search.  What is added:
//   - the automaton is deterministic, so a prefix has exactly ONE state: two beams with the same prefix have the same state and the
//     exact merge stays valid unchanged.  Each beam carries its LOCAL state (one more int[KMAX] per beam buffer).
//   - line b searches under automaton w = which[b]: rows g_state_off[w] .. g_state_off[w+1] of dfa_next[states][V] (the local state
//     after class c, -1: no arc) and dfa_dist[states] (the fewest symbols from the state to an accepting one; 0 exactly for the
//     accepting states, so there is no accept array).
//   - at frame t with rem = len - 1 - t frames left after it, an extension of beam k by class c is a candidate only if
//     n = dfa_next[state_k][c] is a state of the automaton and 0 <= dfa_dist[n] <= rem; a stay only if 0 <= dfa_dist[state_k] <= rem.
//     Every other candidate is -inf, which top_k never takes.  Every further symbol needs a frame of its own, so a prefix that
//     fails the test has no accepted completion in the frames left: the rule removes only dead prefixes (it is a lower bound: it
//     ignores the blank a repeated symbol needs, so some dead prefixes stay, but no live one goes).  At the last frame rem = 0 and
//     only accepting states survive; the final ranking filters on dfa_dist == 0 all the same (a line of no frames never gets here).
//   - the beam may run empty mid-line (the language needs more symbols than there are frames): the ranks then stay unfilled.
// Device contents are never trusted and never become a load address unchecked: which[b] outside [0, g), an empty or reversed state
// range or one past g_state_off[g] gives that line no hypothesis; a next state outside the automaton's range is no arc; a negative
// distance is "cannot accept".  (g_state_off[g] itself is the size of the two tables and must be right, as lm_states must.)
//
// LDS: the beam buffers grow by 2 * 512 bytes and the per-beam viability flags take 512 more, so the static part is 22 592 bytes
// against ctc_beam.hip's 21 056; with the worst-case 128 KiB of candidate scores (K = 128, V = 256) that is 153 664 bytes, about
// 150.1 KiB of the 160 KiB per CU.  One line per CU, as before.
#include "ctc_beam_common.h"

namespace {

using namespace ctcbeam;

struct GBeamBuf {
    float pb[KMAX], pnb[KMAX], acc[KMAX];
    int last[KMAX], len[KMAX], lms[KMAX], node[KMAX], gst[KMAX];
    unsigned long long hash[KMAX], phash[KMAX];
};

__global__ __launch_bounds__(BT) void ctc_grammar_beam_kernel(
    const float* __restrict__ logits, const int32_t* __restrict__ lens, int T, int B, int V, const int32_t* __restrict__ canon, int K,
    int nbest, const int32_t* __restrict__ g_state_off, const int32_t* __restrict__ dfa_next, const int32_t* __restrict__ dfa_dist, int G,
    const int32_t* __restrict__ which, const float* __restrict__ lm_logp, const int32_t* __restrict__ lm_next,
    const float* __restrict__ lm_eos, int S, int lm_start, float alpha, float beta, float prune, int32_t* __restrict__ out_labels,
    int32_t* __restrict__ out_lens, float* __restrict__ out_scores, int2* __restrict__ pool_all) {
    extern __shared__ float s_score[];                 // [K*V]
    __shared__ GBeamBuf s_beam[2];
    __shared__ Frame s_f;
    __shared__ Select s_sel;
    __shared__ float s_spb[KMAX], s_spnb[KMAX], s_fin[KMAX];
    __shared__ int s_merge[KMAX], s_ok[KMAX];

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const bool has_lm = lm_logp != nullptr;
    const int start = has_lm ? lm_start : 0;
    const int len_b = min(max(lens[b], 0), T);
    int2* pool = pool_all + (long)b * T * K;

    // the line's automaton: rows s0 .. s0 + ns of the tables, or none (the whole workgroup takes the same way)
    const int w = which ? which[b] : 0;
    int s0 = 0, ns = 0;
    if (w >= 0 && w < G) {
        const int total = g_state_off[G], lo = g_state_off[w], hi = g_state_off[w + 1];
        if (lo >= 0 && hi > lo && hi <= total) { s0 = lo; ns = hi - lo; }
    }
    if (ns == 0) {
        if (tid < nbest) write_hyp(b, tid, nbest, T, false, 0, -1, 0.f, 0.f, 0.f, pool, T * K, out_labels, out_lens, out_scores);
        return;
    }
    const int32_t* __restrict__ g_next = dfa_next + (long)s0 * V;
    const int32_t* __restrict__ g_dist = dfa_dist + s0;

    init_classes(canon, V, s_f);
    if (tid == 0) {
        GBeamBuf& B0 = s_beam[0];
        B0.pb[0] = 0.f; B0.pnb[0] = NEG_INF; B0.acc[0] = 0.f; B0.last[0] = -1; B0.len[0] = 0; B0.lms[0] = start;
        B0.node[0] = -1; B0.gst[0] = 0; B0.hash[0] = HASH_ROOT; B0.phash[0] = 0;
    }
    int cur = 0, nb = 1;
    __syncthreads();

    for (int t = 0; t < len_b && nb > 0; ++t) {
        const GBeamBuf& C = s_beam[cur];
        GBeamBuf& N = s_beam[cur ^ 1];
        const int rem = len_b - 1 - t;
        // 1. log-softmax of the row, class log-probs
        frame_logprobs(logits + ((long)t * B + b) * V, V, prune, s_f);

        // 2. stay probabilities and the merge of the extension that re-creates beam j from its parent prefix; whether j may stay
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
            const int dj = g_dist[C.gst[j]];
            s_ok[j] = (dj >= 0 && dj <= rem) ? 1 : 0;
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
                if (!s_ok[k]) sc = NEG_INF;
            } else {
                const float xp = s_f.xp[c];
                if (xp == NEG_INF) {
                    sc = NEG_INF;
                } else {
                    const float pnb = ((c == C.last[k]) ? C.pb[k] : lse2(C.pb[k], C.pnb[k])) + xp;
                    const float lmv = has_lm ? C.acc[k] + lm_logp[(long)C.lms[k] * V + c] : 0.f;
                    sc = pnb + (has_lm && alpha != 0.f ? alpha * lmv : 0.f) + beta * (float)(C.len[k] + 1);
                    const int n = g_next[(long)C.gst[k] * V + c];
                    const int dn = (n >= 0 && n < ns) ? g_dist[n] : -1;
                    if (!(dn >= 0 && dn <= rem)) sc = NEG_INF;
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
                N.lms[q] = C.lms[k]; N.node[q] = C.node[k]; N.gst[q] = C.gst[k]; N.hash[q] = C.hash[k]; N.phash[q] = C.phash[k];
            } else {
                const int node = t * K + q;
                N.pb[q] = NEG_INF;
                N.pnb[q] = ((c == C.last[k]) ? C.pb[k] : lse2(C.pb[k], C.pnb[k])) + s_f.xp[c];
                if (has_lm) {
                    const long e = (long)C.lms[k] * V + c;
                    const int ls = lm_next[e];
                    N.acc[q] = C.acc[k] + lm_logp[e];
                    N.lms[q] = (ls >= 0 && ls < S) ? ls : start;
                } else {
                    N.acc[q] = 0.f;
                    N.lms[q] = 0;
                }
                const int n = g_next[(long)C.gst[k] * V + c];
                N.gst[q] = (n >= 0 && n < ns) ? n : 0;           // a kept candidate has passed the test above
                N.last[q] = c; N.len[q] = C.len[k] + 1; N.node[q] = node;
                N.hash[q] = hash_push(C.hash[k], c); N.phash[q] = C.hash[k];
                pool[node] = make_int2(C.node[k], c);
            }
        }
        nb = nsel;
        cur ^= 1;
        __syncthreads();
    }

    // end of line: accepting beams only, + alpha * ln P(</s> | state), final ranking (ties: the rank at the last frame; a beam that
    // does not accept ranks behind every one that does), backtrack the top nbest
    const GBeamBuf& C = s_beam[cur];
    if (tid < nb) {
        const float lmt = has_lm ? C.acc[tid] + lm_eos[C.lms[tid]] : 0.f;
        s_spb[tid] = lse2(C.pb[tid], C.pnb[tid]);
        s_spnb[tid] = lmt;
        const float fin = s_spb[tid] + (has_lm && alpha != 0.f ? alpha * lmt : 0.f) + beta * (float)C.len[tid];
        const bool accepts = g_dist[C.gst[tid]] == 0;
        s_ok[tid] = accepts ? 1 : 0;
        s_fin[tid] = accepts ? fin : __uint_as_float(0x7fc00000u);
    }
    __syncthreads();
    rank_final(s_fin, nb, s_sel.order);
    if (tid < nbest) {
        const int q = tid;
        const int j = q < nb ? s_sel.order[q] : 0;
        write_hyp(b, q, nbest, T, q < nb && s_ok[j] != 0, C.len[j], C.node[j], s_fin[j], s_spb[j], s_spnb[j], pool, T * K, out_labels,
                  out_lens, out_scores);
    }
}

}  // namespace

extern "C" size_t vocr_ctc_grammar_beam_workspace_bytes(int t, int b, int v, int beam, int nbest) {
    if (t <= 0 || b <= 0 || v <= 0 || v > VMAX || beam < 1 || beam > KMAX || nbest < 1 || nbest > beam) return 0;
    if ((long)t * b * beam >= (1L << 31) || (long)t * beam >= (1L << 30)) return 0;
    return (size_t)t * b * beam * sizeof(int2);
}

extern "C" int vocr_ctc_grammar_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam,
                                            int nbest, const int32_t* g_state_off, const int32_t* dfa_next, const int32_t* dfa_dist, int g,
                                            const int32_t* which, const float* lm_logp, const int32_t* lm_next, const float* lm_eos,
                                            int lm_states, int lm_start, float lm_weight, float insertion_bonus, float prune_logp,
                                            int32_t* out_labels, int32_t* out_lens, float* out_scores, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    VOCR_CHECK_ARG(logits && lens && out_labels && out_lens && out_scores && workspace, "vocr_ctc_grammar_beam_search: null pointer");
    VOCR_CHECK_ARG(g_state_off && dfa_next && dfa_dist && which, "vocr_ctc_grammar_beam_search: null automaton table or which");
    VOCR_CHECK_ARG(g >= 1, "vocr_ctc_grammar_beam_search: need g >= 1 (g=%d)", g);
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 0 && v <= VMAX, "vocr_ctc_grammar_beam_search: need t > 0, b > 0, 1 <= v <= %d (t=%d b=%d v=%d)",
                   VMAX, t, b, v);
    VOCR_CHECK_ARG(beam >= 1 && beam <= KMAX, "vocr_ctc_grammar_beam_search: need 1 <= beam <= %d (beam=%d)", KMAX, beam);
    VOCR_CHECK_ARG(nbest >= 1 && nbest <= beam, "vocr_ctc_grammar_beam_search: need 1 <= nbest <= beam (nbest=%d beam=%d)", nbest, beam);
    VOCR_CHECK_ARG((long)t * b * beam < (1L << 31) && (long)t * beam < (1L << 30), "vocr_ctc_grammar_beam_search: t*b*beam too large");
    const bool any_lm = lm_logp || lm_next || lm_eos;
    VOCR_CHECK_ARG(!any_lm || (lm_logp && lm_next && lm_eos), "vocr_ctc_grammar_beam_search: lm_logp, lm_next and lm_eos go together");
    VOCR_CHECK_ARG(!any_lm || (lm_states >= 1 && lm_start >= 0 && lm_start < lm_states),
                   "vocr_ctc_grammar_beam_search: need 0 <= lm_start < lm_states (lm_start=%d lm_states=%d)", lm_start, lm_states);
    VOCR_CHECK_ARG(__builtin_isfinite(lm_weight) && __builtin_isfinite(insertion_bonus) && !__builtin_isnan(prune_logp),
                   "vocr_ctc_grammar_beam_search: lm_weight and insertion_bonus must be finite, prune_logp not NaN");
    const size_t need = vocr_ctc_grammar_beam_workspace_bytes(t, b, v, beam, nbest);
    VOCR_CHECK_ARG(need > 0 && workspace_bytes >= need, "vocr_ctc_grammar_beam_search: workspace too small (%zu < %zu bytes)",
                   workspace_bytes, need);
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_grammar_beam_kernel};
    if (vocr_allow_dynamic_lds(big, 1, KMAX * VMAX * (int)sizeof(float), &lds_set, "vocr_ctc_grammar_beam_search") != VOCR_OK)
        return VOCR_ELAUNCH;
    const size_t lds = (size_t)beam * v * sizeof(float);
    ctc_grammar_beam_kernel<<<b, BT, lds, (hipStream_t)stream>>>(logits, lens, t, b, v, canon, beam, nbest, g_state_off, dfa_next, dfa_dist,
                                                                 g, which, any_lm ? lm_logp : nullptr, lm_next, lm_eos,
                                                                 any_lm ? lm_states : 1, any_lm ? lm_start : 0, lm_weight,
                                                                 insertion_bonus, prune_logp, out_labels, out_lens, out_scores,
                                                                 (int2*)workspace);
    VOCR_CHECK_LAUNCH("vocr_ctc_grammar_beam_search");
    return VOCR_OK;
}
