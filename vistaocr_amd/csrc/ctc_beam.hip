// CTC prefix beam search with an optional character n-gram LM: the search side of the reference's decode_with_lm
// (src/decoder.py:11-109, src/models/cnnlstm.py:298-475), with a character n-gram in ARPA form standing in for the eesen WFST.
// ONE kernel, template <bool GRAMMAR>, behind two entries: vocr_ctc_beam_search (false) and vocr_ctc_grammar_beam_search (true: the
// same search over the labellings that a deterministic finite automaton ACCEPTS; "The grammar" below).
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
// their LM loads) per pass or merging K sorted per-beam lists.
//
// LM: backoff-resolved dense tables over S states, lm_logp[S][V] (natural log), lm_next[S][V], lm_eos[S]; a candidate costs one
// load of each, coalesced over c.  State indices read from lm_next outside [0, S) fall back to lm_start (never an out-of-range load).
// prune_logp: classes whose frame log-prob is below it are not extended (-inf: off, the exact search).
//
// The grammar (GRAMMAR = true).  vocr_ctc_grammar_scores says how probable it is that a line belongs to a regular language and returns
// the best single PATH; this search sums the paths of each labelling, as the character and word searches do, and keeps only prefixes the
// automaton can still complete.  Everything above is the same code, so under the one-state automaton that accepts everything the
// search takes the decisions of vocr_ctc_beam_search, bit for bit.  What `if constexpr (GRAMMAR)` adds, and only there (the false
// instantiation has none of it, not as a branch either: no state array, no flags, no automaton arguments):
//   - the automaton is deterministic, so a prefix has exactly ONE state: two beams with the same prefix have the same state and the
//     exact merge stays valid unchanged.  Each beam carries its LOCAL state (one more int[KMAX] per beam buffer: BeamState<true>).
//   - line b searches under automaton w = which[b]: rows state_off[w] .. state_off[w+1] of next[states][V] (the local state after
//     class c, -1: no arc) and dist[states] (the fewest symbols from the state to an accepting one; 0 exactly for the accepting
//     states, so there is no accept array).
//   - at frame t with rem = len - 1 - t frames left after it, an extension of beam k by class c is a candidate only if
//     n = next[state_k][c] is a state of the automaton and 0 <= dist[n] <= rem; a stay only if 0 <= dist[state_k] <= rem.
//     Every other candidate is -inf, which top_k never takes.  Every further symbol needs a frame of its own, so a prefix that
//     fails the test has no accepted completion in the frames left: the rule removes only dead prefixes (it is a lower bound: it
//     ignores the blank a repeated symbol needs, so some dead prefixes stay, but no live one goes).  At the last frame rem = 0 and
//     only accepting states survive; the final ranking filters on dist == 0 all the same (a line of no frames never gets here).
//   - the beam may run empty mid-line (the language needs more symbols than there are frames): the frame loop ends and the ranks
//     stay unfilled.
//
// The weighted grammar (GRAMMAR = WEIGHTED = true, vocr_ctc_grammar_beam_search_weighted).  The automaton's arcs and accepting states
// carry natural-log weights, logw[states][V] in next's indexing and final[states].  The automaton is deterministic, so a prefix has
// one state AND one accumulated weight: the exact merge stays valid for the reason the character n-gram's does.  What `if constexpr
// (WEIGHTED)` adds, and only there:
//   - each beam carries gacc, the sum of the weights of its prefix's arcs (one more float[KMAX] per beam buffer);
//   - a candidate's rank adds grammar_weight * gacc_k (a stay) or grammar_weight * (gacc_k + logw[state_k][c]) (an extension), between
//     the LM term and the insertion bonus - so that Grammar.from_ngram's tables under grammar_weight = alpha, without an LM, add up in
//     the order of vocr_ctc_beam_search with that LM under lm_weight = alpha;
//   - the final rank adds grammar_weight * (gacc + final[state]), and that sum, unscaled, is the hypothesis's out_grammar;
//   - an arc whose weight is NaN or infinite is no arc, and an accepting state with such a final weight does not accept.
// The distance rule, the merge, top-K and the total order are untouched.
//
// Device contents are never trusted and never become a load address unchecked: which[b] outside [0, g), an empty or reversed state
// range or one past state_off[g] gives that line no hypothesis; a next state outside the automaton's range is no arc; a negative
// distance is "cannot accept".  (state_off[g] itself is the size of the two tables and must be right, as lm_states must.)
//
// LDS: static 21 056 bytes without the grammar (two beam-state buffers, class log-probs, histogram, selection); with it the beam
// buffers grow by 2 * 512 bytes and the per-beam viability flags take 512 more: 22 592; with weights the buffers grow by 2 * 512 again:
// 23 616.  With the worst-case 128 KiB of candidate scores (K = 128, V = 256) that is 152 128, 153 664 and 154 688 bytes, about 148.6,
// 150.1 and 151.1 KiB of the 160 KiB per CU: one line per CU, which is what the problem has (B lines << 256 CUs).
//
// Steps 1, 2, 4 and the backtrack are the device functions of ctc_beam_common.h, shared with the word search (ctc_word_beam.hip), as
// are the host checks of the entries; this file holds the character LM's candidate scoring, the beam state and the grammar.
#include "ctc_beam_common.h"

namespace {

using namespace ctcbeam;

// What the grammar adds to a beam buffer and to the kernel's arguments; both empty without it.
template <bool GRAMMAR, bool WEIGHTED>
struct BeamState {};
template <>
struct BeamState<true, false> {
    int gst[KMAX];                              // the beam's local automaton state
};
template <>
struct BeamState<true, true> : BeamState<true, false> {
    float gacc[KMAX];                           // the accumulated weight of the prefix's arcs
};

template <bool GRAMMAR, bool WEIGHTED>
struct Dfa {};
template <>
struct Dfa<true, false> {
    const int32_t* __restrict__ state_off;      // [G+1]
    const int32_t* __restrict__ next;           // [states][V]
    const int32_t* __restrict__ dist;           // [states]
    const int32_t* __restrict__ which;          // [B]
    int G;
};
template <>
struct Dfa<true, true> : Dfa<true, false> {
    const float* __restrict__ logw;             // [states][V], next's indexing
    const float* __restrict__ fin;              // [states]
    float weight;                               // grammar_weight
    float* __restrict__ out_grammar;            // [B][nbest] or NULL
};

__device__ __forceinline__ bool w_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

template <bool GRAMMAR, bool WEIGHTED>
struct BeamBuf : BeamState<GRAMMAR, WEIGHTED> {
    float pb[KMAX], pnb[KMAX], acc[KMAX];
    int last[KMAX], len[KMAX], lms[KMAX], node[KMAX];
    unsigned long long hash[KMAX], phash[KMAX];
};

template <bool GRAMMAR, bool WEIGHTED>
__global__ __launch_bounds__(BT) void ctc_beam_kernel(const float* __restrict__ logits, const int32_t* __restrict__ lens, int T, int B,
                                                      int V, const int32_t* __restrict__ canon, int K, int nbest, Dfa<GRAMMAR, WEIGHTED> D,
                                                      const float* __restrict__ lm_logp, const int32_t* __restrict__ lm_next,
                                                      const float* __restrict__ lm_eos, int S, int lm_start, float alpha, float beta,
                                                      float prune, int32_t* __restrict__ out_labels, int32_t* __restrict__ out_lens,
                                                      float* __restrict__ out_scores, int2* __restrict__ pool_all) {
    extern __shared__ float s_score[];                 // [K*V]
    __shared__ BeamBuf<GRAMMAR, WEIGHTED> s_beam[2];
    __shared__ Frame s_f;
    __shared__ Select s_sel;
    __shared__ float s_spb[KMAX], s_spnb[KMAX], s_fin[KMAX];
    __shared__ int s_merge[KMAX];
    __shared__ int s_ok[KMAX];                         // GRAMMAR: beam j may stay / accepts; never referenced, so not allocated, without

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const bool has_lm = lm_logp != nullptr;
    const int start = has_lm ? lm_start : 0;
    const int len_b = min(max(lens[b], 0), T);
    int2* pool = pool_all + (long)b * T * K;

    // GRAMMAR: the line's automaton, rows s0 .. s0 + ns of the tables, or none (the whole workgroup takes the same way)
    const int32_t* g_next = nullptr;
    const int32_t* g_dist = nullptr;
    const float* g_logw = nullptr;                     // WEIGHTED: the same rows of the weight tables
    const float* g_fin = nullptr;
    int ns = 0;
    if constexpr (GRAMMAR) {
        const int w = D.which ? D.which[b] : 0;
        int s0 = 0;
        if (w >= 0 && w < D.G) {
            const int total = D.state_off[D.G], lo = D.state_off[w], hi = D.state_off[w + 1];
            if (lo >= 0 && hi > lo && hi <= total) { s0 = lo; ns = hi - lo; }
        }
        if (ns == 0) {
            if (tid < nbest) {
                write_hyp(b, tid, nbest, T, false, 0, -1, 0.f, 0.f, 0.f, pool, T * K, out_labels, out_lens, out_scores);
                if constexpr (WEIGHTED) {
                    if (D.out_grammar) D.out_grammar[(long)b * nbest + tid] = 0.f;
                }
            }
            return;
        }
        g_next = D.next + (long)s0 * V;
        g_dist = D.dist + s0;
        if constexpr (WEIGHTED) {
            g_logw = D.logw + (long)s0 * V;
            g_fin = D.fin + s0;
        }
    }

    init_classes(canon, V, s_f);
    if (tid == 0) {
        BeamBuf<GRAMMAR, WEIGHTED>& B0 = s_beam[0];
        B0.pb[0] = 0.f; B0.pnb[0] = NEG_INF; B0.acc[0] = 0.f; B0.last[0] = -1; B0.len[0] = 0; B0.lms[0] = start;
        B0.node[0] = -1; B0.hash[0] = HASH_ROOT; B0.phash[0] = 0;
        if constexpr (GRAMMAR) B0.gst[0] = 0;
        if constexpr (WEIGHTED) B0.gacc[0] = 0.f;
    }
    int cur = 0, nb = 1;
    __syncthreads();

    for (int t = 0; t < len_b && (!GRAMMAR || nb > 0); ++t) {
        const BeamBuf<GRAMMAR, WEIGHTED>& C = s_beam[cur];
        BeamBuf<GRAMMAR, WEIGHTED>& N = s_beam[cur ^ 1];
        const int rem = len_b - 1 - t;                 // GRAMMAR: the frames left after this one
        // 1. log-softmax of the row, class log-probs
        frame_logprobs(logits + ((long)t * B + b) * V, V, prune, s_f);

        // 2. stay probabilities and the merge of the extension that re-creates beam j from its parent prefix; whether j may stay
        if (tid < nb) {
            stay_and_merge(C, tid, nb, s_f, pool, T * K, s_merge, s_spb, s_spnb);
            if constexpr (GRAMMAR) {
                const int dj = g_dist[C.gst[tid]];
                s_ok[tid] = (dj >= 0 && dj <= rem) ? 1 : 0;
            }
        }
        __syncthreads();

        // 3. candidate scores
        const int ncand = nb * V;
        for (int i = tid; i < ncand; i += BT) {
            const int k = i / V, c = i - k * V;
            float sc;
            if (c == 0) {
                const float ac = lse2(s_spb[k], s_spnb[k]);
                if constexpr (WEIGHTED)
                    sc = ac + (has_lm && alpha != 0.f ? alpha * C.acc[k] : 0.f) + D.weight * C.gacc[k] + beta * (float)C.len[k];
                else
                    sc = ac + (has_lm && alpha != 0.f ? alpha * C.acc[k] : 0.f) + beta * (float)C.len[k];
                if constexpr (GRAMMAR) {
                    if (!s_ok[k]) sc = NEG_INF;
                }
            } else {
                const float xp = s_f.xp[c];
                if (xp == NEG_INF) {
                    sc = NEG_INF;
                } else {
                    const float pnb = ((c == C.last[k]) ? C.pb[k] : lse2(C.pb[k], C.pnb[k])) + xp;
                    const float lmv = has_lm ? C.acc[k] + lm_logp[(long)C.lms[k] * V + c] : 0.f;
                    if constexpr (!WEIGHTED) sc = pnb + (has_lm && alpha != 0.f ? alpha * lmv : 0.f) + beta * (float)(C.len[k] + 1);
                    if constexpr (GRAMMAR) {
                        const int n = g_next[(long)C.gst[k] * V + c];
                        const int dn = (n >= 0 && n < ns) ? g_dist[n] : -1;
                        if constexpr (WEIGHTED) {
                            const float w = (dn >= 0 && dn <= rem) ? g_logw[(long)C.gst[k] * V + c] : 0.f;
                            sc = pnb + (has_lm && alpha != 0.f ? alpha * lmv : 0.f) + D.weight * (C.gacc[k] + w) +
                                 beta * (float)(C.len[k] + 1);
                            if (!w_finite(w)) sc = NEG_INF;
                        }
                        if (!(dn >= 0 && dn <= rem)) sc = NEG_INF;
                    }
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
                if constexpr (GRAMMAR) N.gst[q] = C.gst[k];
                if constexpr (WEIGHTED) N.gacc[q] = C.gacc[k];
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
                if constexpr (GRAMMAR) {
                    const int n = g_next[(long)C.gst[k] * V + c];
                    N.gst[q] = (n >= 0 && n < ns) ? n : 0;       // a kept candidate has passed the test above
                    if constexpr (WEIGHTED) N.gacc[q] = C.gacc[k] + g_logw[(long)C.gst[k] * V + c];
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

    // end of line: + alpha * ln P(</s> | state), final ranking (ties: the rank at the last frame), backtrack the top nbest.  GRAMMAR:
    // accepting beams only (a beam that does not accept ranks behind every one that does)
    const BeamBuf<GRAMMAR, WEIGHTED>& C = s_beam[cur];
    if (tid < nb) {
        const float lmt = has_lm ? C.acc[tid] + lm_eos[C.lms[tid]] : 0.f;
        s_spb[tid] = lse2(C.pb[tid], C.pnb[tid]);
        s_spnb[tid] = lmt;
        float fin;
        if constexpr (WEIGHTED)
            fin = s_spb[tid] + (has_lm && alpha != 0.f ? alpha * lmt : 0.f) + D.weight * (C.gacc[tid] + g_fin[C.gst[tid]]) +
                  beta * (float)C.len[tid];
        else
            fin = s_spb[tid] + (has_lm && alpha != 0.f ? alpha * lmt : 0.f) + beta * (float)C.len[tid];
        if constexpr (GRAMMAR) {
            bool accepts = g_dist[C.gst[tid]] == 0;
            if constexpr (WEIGHTED) accepts = accepts && w_finite(g_fin[C.gst[tid]]);
            s_ok[tid] = accepts ? 1 : 0;
            s_fin[tid] = accepts ? fin : __uint_as_float(0x7fc00000u);
        } else {
            s_fin[tid] = fin;
        }
    }
    __syncthreads();
    rank_final(s_fin, nb, s_sel.order);
    if (tid < nbest) {
        const int q = tid;
        const int j = q < nb ? s_sel.order[q] : 0;
        bool keep = q < nb;
        if constexpr (GRAMMAR) keep = keep && s_ok[j] != 0;
        write_hyp(b, q, nbest, T, keep, C.len[j], C.node[j], s_fin[j], s_spb[j], s_spnb[j], pool, T * K, out_labels, out_lens,
                  out_scores);
        if constexpr (WEIGHTED) {
            if (D.out_grammar) D.out_grammar[(long)b * nbest + q] = keep ? C.gacc[j] + g_fin[C.gst[j]] : 0.f;
        }
    }
}

// the character LM's arguments and the two weights, under the entry's name
int check_char_lm(const char* who, const float* lm_logp, const int32_t* lm_next, const float* lm_eos, int lm_states, int lm_start,
                  float lm_weight, float insertion_bonus, float prune_logp) {
    const bool any_lm = lm_logp || lm_next || lm_eos;
    VOCR_CHECK_ARG(!any_lm || (lm_logp && lm_next && lm_eos), "%s: lm_logp, lm_next and lm_eos go together", who);
    VOCR_CHECK_ARG(!any_lm || (lm_states >= 1 && lm_start >= 0 && lm_start < lm_states),
                   "%s: need 0 <= lm_start < lm_states (lm_start=%d lm_states=%d)", who, lm_start, lm_states);
    VOCR_CHECK_ARG(__builtin_isfinite(lm_weight) && __builtin_isfinite(insertion_bonus) && !__builtin_isnan(prune_logp),
                   "%s: lm_weight and insertion_bonus must be finite, prune_logp not NaN", who);
    return VOCR_OK;
}

// what both entries do once the automaton, if any, has passed: the checks, the launch of their instantiation
template <bool GRAMMAR, bool WEIGHTED>
int search(const char* who, size_t need, const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam,
           int nbest, Dfa<GRAMMAR, WEIGHTED> D, const float* lm_logp, const int32_t* lm_next, const float* lm_eos, int lm_states, int lm_start,
           float lm_weight, float insertion_bonus, float prune_logp, int32_t* out_labels, int32_t* out_lens, float* out_scores,
           void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = check_char_lm(who, lm_logp, lm_next, lm_eos, lm_states, lm_start, lm_weight, insertion_bonus, prune_logp)) return rc;
    static VocrPerDevice lds_set;
    if (const int rc = check_search_args(who, logits, lens, t, b, v, beam, nbest, out_labels, out_lens, out_scores, workspace,
                                         workspace_bytes, need, (const void*)ctc_beam_kernel<GRAMMAR, WEIGHTED>, &lds_set))
        return rc;
    const bool any_lm = lm_logp != nullptr;
    const size_t lds = (size_t)beam * v * sizeof(float);
    ctc_beam_kernel<GRAMMAR, WEIGHTED><<<b, BT, lds, (hipStream_t)stream>>>(logits, lens, t, b, v, canon, beam, nbest, D, lm_logp, lm_next,
                                                                             lm_eos, any_lm ? lm_states : 1, any_lm ? lm_start : 0,
                                                                             lm_weight, insertion_bonus, prune_logp, out_labels, out_lens,
                                                                             out_scores, (int2*)workspace);
    VOCR_CHECK_LAUNCH(who);
    return VOCR_OK;
}

}  // namespace

extern "C" size_t vocr_ctc_beam_workspace_bytes(int t, int b, int v, int beam, int nbest) {
    if (t <= 0 || b <= 0 || v <= 0 || v > VMAX || beam < 1 || beam > KMAX || nbest < 1 || nbest > beam) return 0;
    return (size_t)t * b * beam * sizeof(int2);
}

extern "C" size_t vocr_ctc_grammar_beam_workspace_bytes(int t, int b, int v, int beam, int nbest) {
    const size_t need = vocr_ctc_beam_workspace_bytes(t, b, v, beam, nbest);
    if (need == 0 || (long)t * b * beam >= (1L << 31) || (long)t * beam >= (1L << 30)) return 0;
    return need;
}

extern "C" int vocr_ctc_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam,
                                    int nbest, const float* lm_logp, const int32_t* lm_next, const float* lm_eos, int lm_states,
                                    int lm_start, float lm_weight, float insertion_bonus, float prune_logp, int32_t* out_labels,
                                    int32_t* out_lens, float* out_scores, void* workspace, size_t workspace_bytes, void* stream) {
    return search<false, false>("vocr_ctc_beam_search", vocr_ctc_beam_workspace_bytes(t, b, v, beam, nbest), logits, lens, t, b, v, canon, beam,
                         nbest, {}, lm_logp, lm_next, lm_eos, lm_states, lm_start, lm_weight, insertion_bonus, prune_logp, out_labels,
                         out_lens, out_scores, workspace, workspace_bytes, stream);
}

extern "C" int vocr_ctc_grammar_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam,
                                            int nbest, const int32_t* g_state_off, const int32_t* dfa_next, const int32_t* dfa_dist, int g,
                                            const int32_t* which, const float* lm_logp, const int32_t* lm_next, const float* lm_eos,
                                            int lm_states, int lm_start, float lm_weight, float insertion_bonus, float prune_logp,
                                            int32_t* out_labels, int32_t* out_lens, float* out_scores, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    VOCR_CHECK_ARG(g_state_off && dfa_next && dfa_dist && which, "vocr_ctc_grammar_beam_search: null automaton table or which");
    VOCR_CHECK_ARG(g >= 1, "vocr_ctc_grammar_beam_search: need g >= 1 (g=%d)", g);
    return search<true, false>("vocr_ctc_grammar_beam_search", vocr_ctc_grammar_beam_workspace_bytes(t, b, v, beam, nbest), logits, lens, t,
                               b, v, canon, beam, nbest, {g_state_off, dfa_next, dfa_dist, which, g}, lm_logp, lm_next, lm_eos, lm_states,
                               lm_start, lm_weight, insertion_bonus, prune_logp, out_labels, out_lens, out_scores, workspace,
                               workspace_bytes, stream);
}

extern "C" int vocr_ctc_grammar_beam_search_weighted(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                                     int beam, int nbest, const int32_t* g_state_off, const int32_t* dfa_next,
                                                     const int32_t* dfa_dist, const float* dfa_logw, const float* dfa_final, int g,
                                                     const int32_t* which, const float* lm_logp, const int32_t* lm_next,
                                                     const float* lm_eos, int lm_states, int lm_start, float lm_weight,
                                                     float grammar_weight, float insertion_bonus, float prune_logp, int32_t* out_labels,
                                                     int32_t* out_lens, float* out_scores, float* out_grammar, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    const char* who = "vocr_ctc_grammar_beam_search_weighted";
    VOCR_CHECK_ARG(g_state_off && dfa_next && dfa_dist && which, "%s: null automaton table or which", who);
    VOCR_CHECK_ARG(g >= 1, "%s: need g >= 1 (g=%d)", who, g);
    VOCR_CHECK_ARG(!dfa_logw == !dfa_final, "%s: dfa_logw and dfa_final go together (dfa_logw %s, dfa_final %s)", who,
                   dfa_logw ? "given" : "NULL", dfa_final ? "given" : "NULL");
    VOCR_CHECK_ARG(__builtin_isfinite(grammar_weight), "%s: grammar_weight must be finite", who);
    const size_t need = vocr_ctc_grammar_beam_workspace_bytes(t, b, v, beam, nbest);
    if (!dfa_logw) {                                   // no weights: the unweighted instantiation, every hypothesis's grammar weight 0
        const int rc = search<true, false>(who, need, logits, lens, t, b, v, canon, beam, nbest, {g_state_off, dfa_next, dfa_dist, which, g},
                                           lm_logp, lm_next, lm_eos, lm_states, lm_start, lm_weight, insertion_bonus, prune_logp,
                                           out_labels, out_lens, out_scores, workspace, workspace_bytes, stream);
        if (rc == VOCR_OK && out_grammar &&
            hipMemsetAsync(out_grammar, 0, (size_t)b * nbest * sizeof(float), (hipStream_t)stream) != hipSuccess) {
            vocr_set_error("%s: hipMemsetAsync failed", who);
            return VOCR_ELAUNCH;
        }
        return rc;
    }
    Dfa<true, true> D;
    D.state_off = g_state_off; D.next = dfa_next; D.dist = dfa_dist; D.which = which; D.G = g;
    D.logw = dfa_logw; D.fin = dfa_final; D.weight = grammar_weight; D.out_grammar = out_grammar;
    return search<true, true>(who, need, logits, lens, t, b, v, canon, beam, nbest, D, lm_logp, lm_next, lm_eos, lm_states, lm_start,
                              lm_weight, insertion_bonus, prune_logp, out_labels, out_lens, out_scores, workspace, workspace_bytes,
                              stream);
}
