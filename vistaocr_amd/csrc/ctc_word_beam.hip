// CTC prefix beam search scored by a WORD n-gram with a lexicon: the stand-in for the reference's TLG.fst decode (decode_with_lm,
// src/decoder.py:11-109), whose lexicon limits the output to dictionary words and whose G is a word n-gram over the tokens of
// form_tokenized_words (src/textutils.py:290-323).
//
// The search is ctc_beam.hip's (ctc_beam_common.h: classes, exact merge, radix top-K under the total order (score desc, slot id
// k*V + c), final ranking, backtrack); what differs is the per-beam state and the candidate scoring.  Every non-blank class has a
// kind: LETTER (runs of letters are words), SPACE (u0020: separates tokens) or SINGLE (a punctuation mark or digit: a token of its
// own, tok[c] its LM token).  A beam is outside a word (wn = -1), inside an open word at trie node wn >= 0, or in the OOV state
// (wn = -2: the open word has left the lexicon trie; only with an open vocabulary).  It carries the LM state after its CLOSED tokens
// `lms`, their LM sum `acc`, their count `ntok`, the look-ahead `la` of its open word (0 outside a word; trie_la[wn], the largest
// 1-gram ln P of the lexicon words below the node; ln P_1(<unk>) + oov_penalty for OOV) and, cached when the beam is created since
// they depend on the prefix alone, the close score `clp` / close state `cst` of its open word: ln P(word | lms) for a lexicon word,
// ln P(<unk> | lms) + oov_penalty for any other letter run (-inf with a closed vocabulary).  A candidate (beam k, class c):
//   letter  step the trie from the root or wn; no child: OOV with an open vocabulary, not a candidate with a closed one; OOV stays
//   space   close the open word (acc += clp, lms = cst, ntok += 1), if there is one
//   single  close the open word, if there is one, then acc += ln P(tok[c] | lms) and ntok += 1
// and is ranked by logsumexp(p_b, p_nb) + lm_weight * (acc + la) + word_bonus * ntok.  A candidate whose LM term is -inf is never
// one, whatever lm_weight is (0 * -inf is not formed).  At the end of the line the open word is closed and ln P(</s>) added; a
// beam whose word cannot close is dropped, and a line with no beam left outputs an empty rank with total -inf.
//
// LM tables (vistaocr_amd/lm.py WordNgramLM): the states are every listed history of order < N plus the empty one (state 0), in
// order of their length, so back[s] < s.  State s's successors are off[s]..off[s+1] of succ_tok (sorted) / succ_logp (natural log)
// / succ_next (the longest suffix of h + w that is a state); state 0's list is dense over all W token ids (off[0] = 0, off[1] = W),
// so a unigram is one load.  A lookup binary-searches the state's range; on a miss it adds bow[s] and moves to back[s], ending at
// state 0.  Every index read from a table is range-checked before it is used: a state outside [0, S) or a back[] that does not
// decrease falls back to state 0, a token outside [0, W) is not a candidate, a trie child outside (0, N) is no child.
//
// LDS at K = 128, V = 256: the K*V candidate scores (128 KiB) plus ~27 KiB static (two beam-state buffers of 64 B per beam, the
// frame's class tables, the selection, kinds and tokens per class), within the 160 KiB of a CU.
#include "ctc_beam_common.h"

namespace {

using namespace ctcbeam;

enum { KIND_NONE = 0, KIND_LETTER = 1, KIND_SPACE = 2, KIND_SINGLE = 3 };
constexpr int WN_OUT = -1, WN_OOV = -2;

struct WordBeamBuf {
    float pb[KMAX], pnb[KMAX], acc[KMAX], la[KMAX], clp[KMAX];
    int last[KMAX], len[KMAX], lms[KMAX], node[KMAX], wn[KMAX], ntok[KMAX], cst[KMAX];
    unsigned long long hash[KMAX], phash[KMAX];
};

struct WordLm {
    const int32_t* __restrict__ kind;      // [V]
    const int32_t* __restrict__ tok;       // [V]
    const int32_t* __restrict__ trie_next; // [N][V]
    const int32_t* __restrict__ trie_tok;  // [N]
    const float* __restrict__ trie_la;     // [N]
    const int32_t* __restrict__ off;       // [S+1]
    const int32_t* __restrict__ succ_tok;  // [E]
    const float* __restrict__ succ_logp;   // [E]
    const int32_t* __restrict__ succ_next; // [E]
    const float* __restrict__ bow;         // [S]
    const int32_t* __restrict__ back;      // [S]
    int V, N, S, E, W, start, unk, eos;
    float oov;                             // oov_penalty (-inf: closed vocabulary)
};

// ln P(w | state s) by the ARPA backoff over the CSR tables; *ns = the state after w.
__device__ __forceinline__ float lm_lookup(const WordLm& L, int s, int w, int* ns) {
    if (w < 0 || w >= L.W) { *ns = 0; return NEG_INF; }
    if (s < 0 || s >= L.S) s = 0;
    float add = 0.f;
    while (s > 0) {
        const int lo0 = max(L.off[s], L.W), hi0 = min(L.off[s + 1], L.E);
        int lo = lo0, hi = hi0;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (L.succ_tok[mid] < w) lo = mid + 1; else hi = mid;
        }
        if (lo < hi0 && L.succ_tok[lo] == w) {
            const int n = L.succ_next[lo];
            *ns = (n >= 0 && n < L.S) ? n : 0;
            return add + L.succ_logp[lo];
        }
        add += L.bow[s];
        const int bk = L.back[s];
        s = (bk >= 0 && bk < s) ? bk : 0;
    }
    const int n = L.succ_next[w];
    *ns = (n >= 0 && n < L.S) ? n : 0;
    return add + L.succ_logp[w];
}

// close score and state of an open word at trie node wn (>= 0) or OOV (-2), from LM state s
__device__ __forceinline__ float close_word(const WordLm& L, int wn, int s, int* cs) {
    int t = -1;
    if (wn >= 0) {
        const int tt = L.trie_tok[wn];
        t = (tt >= 0 && tt < L.W) ? tt : -1;
    }
    if (t >= 0) return lm_lookup(L, s, t, cs);
    if (L.oov == NEG_INF) { *cs = s; return NEG_INF; }
    return lm_lookup(L, s, L.unk, cs) + L.oov;
}

// Beam state after extending (wn, acc, lms, ntok, clp, cst) by class c of kind `kd`; false: not a candidate.  With `full` the new
// open word's close score and state are looked up too (only for the kept candidates).
struct Ext {
    float acc, la, clp;
    int wn, lms, ntok, cst;
};

__device__ __forceinline__ bool extend(const WordLm& L, float la_oov, int kd, int c, int wn, float acc, int lms, int ntok, float clp,
                                       int cst, bool full, Ext& e) {
    e.acc = acc; e.lms = lms; e.ntok = ntok; e.la = 0.f; e.wn = WN_OUT; e.clp = 0.f; e.cst = lms;
    if (kd == KIND_LETTER) {
        int nw = WN_OOV;
        if (wn != WN_OOV) {
            const int from = (wn >= 0 && wn < L.N) ? wn : 0;
            const int nx = L.trie_next[(long)from * L.V + c];
            if (nx > 0 && nx < L.N) nw = nx;
        }
        if (nw == WN_OOV) {
            if (L.oov == NEG_INF) return false;
            e.la = la_oov;
            if (wn == WN_OOV) { e.clp = clp; e.cst = cst; full = false; }
        } else {
            e.la = L.trie_la[nw];
        }
        e.wn = nw;
        if (full) e.clp = close_word(L, nw, lms, &e.cst);
        return e.acc + e.la > NEG_INF;
    }
    if (kd != KIND_SPACE && kd != KIND_SINGLE) return false;
    if (wn != WN_OUT) {
        if (!(clp > NEG_INF)) return false;
        e.acc = acc + clp; e.lms = cst; e.ntok = ntok + 1;
    }
    if (kd == KIND_SINGLE) {
        int ns;
        const float lp = lm_lookup(L, e.lms, L.tok[c], &ns);
        if (!(lp > NEG_INF)) return false;
        e.acc += lp; e.lms = ns; e.ntok += 1;
    }
    e.cst = e.lms;
    return e.acc > NEG_INF;
}

__global__ __launch_bounds__(BT) void ctc_word_beam_kernel(const float* __restrict__ logits, const int32_t* __restrict__ lens, int T,
                                                           int B, int V, const int32_t* __restrict__ canon, int K, int nbest, WordLm L,
                                                           float alpha, float beta, int32_t* __restrict__ out_labels,
                                                           int32_t* __restrict__ out_lens, float* __restrict__ out_scores,
                                                           int2* __restrict__ pool_all) {
    extern __shared__ float s_score[];                 // [K*V]
    __shared__ WordBeamBuf s_beam[2];
    __shared__ Frame s_f;
    __shared__ Select s_sel;
    __shared__ float s_spb[KMAX], s_spnb[KMAX], s_fin[KMAX], s_lmt[KMAX];
    __shared__ int s_merge[KMAX];
    __shared__ int s_kind[VMAX], s_tok[VMAX];

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int len_b = min(max(lens[b], 0), T);
    int2* pool = pool_all + (long)b * T * K;
    const bool use_lm = alpha != 0.f;

    init_classes(canon, V, s_f);
    if (tid < V) {
        s_kind[tid] = (tid > 0 && s_f.cls[tid] == tid) ? L.kind[tid] : KIND_NONE;
        s_tok[tid] = L.tok[tid];
    }
    WordLm Ls = L;
    Ls.tok = s_tok;
    int unused;
    const float la_oov = L.oov == NEG_INF ? NEG_INF : lm_lookup(L, 0, L.unk, &unused) + L.oov;
    if (tid == 0) {
        WordBeamBuf& B0 = s_beam[0];
        B0.pb[0] = 0.f; B0.pnb[0] = NEG_INF; B0.acc[0] = 0.f; B0.la[0] = 0.f; B0.clp[0] = 0.f; B0.last[0] = -1; B0.len[0] = 0;
        B0.lms[0] = L.start; B0.node[0] = -1; B0.wn[0] = WN_OUT; B0.ntok[0] = 0; B0.cst[0] = L.start;
        B0.hash[0] = HASH_ROOT; B0.phash[0] = 0;
    }
    int cur = 0, nb = 1;
    __syncthreads();

    for (int t = 0; t < len_b; ++t) {
        const WordBeamBuf& C = s_beam[cur];
        WordBeamBuf& N = s_beam[cur ^ 1];
        frame_logprobs(logits + ((long)t * B + b) * V, V, NEG_INF, s_f);

        if (tid < nb) stay_and_merge(C, tid, nb, s_f, pool, T * K, s_merge, s_spb, s_spnb);
        __syncthreads();

        const int ncand = nb * V;
        for (int i = tid; i < ncand; i += BT) {
            const int k = i / V, c = i - k * V;
            float sc;
            if (c == 0) {
                const float ac = lse2(s_spb[k], s_spnb[k]);
                sc = ac + (use_lm ? alpha * (C.acc[k] + C.la[k]) : 0.f) + beta * (float)C.ntok[k];
            } else {
                const float xp = s_f.xp[c];
                Ext e;
                if (xp == NEG_INF ||
                    !extend(Ls, la_oov, s_kind[c], c, C.wn[k], C.acc[k], C.lms[k], C.ntok[k], C.clp[k], C.cst[k], false, e)) {
                    sc = NEG_INF;
                } else {
                    const float pnb = ((c == C.last[k]) ? C.pb[k] : lse2(C.pb[k], C.pnb[k])) + xp;
                    sc = pnb + (use_lm ? alpha * (e.acc + e.la) : 0.f) + beta * (float)e.ntok;
                }
            }
            s_score[i] = sc;
        }
        __syncthreads();
        if (tid < nb && s_merge[tid] >= 0) s_score[s_merge[tid] * V + C.last[tid]] = NEG_INF;
        __syncthreads();

        const int nsel = top_k(s_score, ncand, K, s_sel);

        if (tid < nsel) {
            const int q = tid, id = s_sel.order[q];
            const int k = id / V, c = id - k * V;
            if (c == 0) {
                N.pb[q] = s_spb[k]; N.pnb[q] = s_spnb[k]; N.acc[q] = C.acc[k]; N.la[q] = C.la[k]; N.clp[q] = C.clp[k];
                N.last[q] = C.last[k]; N.len[q] = C.len[k]; N.lms[q] = C.lms[k]; N.node[q] = C.node[k]; N.wn[q] = C.wn[k];
                N.ntok[q] = C.ntok[k]; N.cst[q] = C.cst[k]; N.hash[q] = C.hash[k]; N.phash[q] = C.phash[k];
            } else {
                Ext e;
                extend(Ls, la_oov, s_kind[c], c, C.wn[k], C.acc[k], C.lms[k], C.ntok[k], C.clp[k], C.cst[k], true, e);
                const int node = t * K + q;
                N.pb[q] = NEG_INF;
                N.pnb[q] = ((c == C.last[k]) ? C.pb[k] : lse2(C.pb[k], C.pnb[k])) + s_f.xp[c];
                N.acc[q] = e.acc; N.la[q] = e.la; N.clp[q] = e.clp; N.lms[q] = e.lms; N.wn[q] = e.wn; N.ntok[q] = e.ntok;
                N.cst[q] = e.cst;
                N.last[q] = c; N.len[q] = C.len[k] + 1; N.node[q] = node;
                N.hash[q] = hash_push(C.hash[k], c); N.phash[q] = C.hash[k];
                pool[node] = make_int2(C.node[k], c);
            }
        }
        nb = nsel;
        cur ^= 1;
        __syncthreads();
    }

    // end of line: close the open word, + ln P(</s>), drop beams whose word cannot close, rank, backtrack the top nbest
    const WordBeamBuf& C = s_beam[cur];
    if (tid < nb) {
        float lmt = C.acc[tid];
        int s = C.lms[tid], nt = C.ntok[tid];
        if (C.wn[tid] != WN_OUT) {
            lmt = C.clp[tid] > NEG_INF ? lmt + C.clp[tid] : NEG_INF;
            s = C.cst[tid];
            nt += 1;
        }
        int unused2;
        if (lmt > NEG_INF) lmt += lm_lookup(L, s, L.eos, &unused2);
        const float ac = lse2(C.pb[tid], C.pnb[tid]);
        s_spb[tid] = ac;
        s_lmt[tid] = lmt;
        s_fin[tid] = lmt > NEG_INF ? ac + (use_lm ? alpha * lmt : 0.f) + beta * (float)nt : NEG_INF;
    }
    __syncthreads();
    rank_final(s_fin, nb, s_sel.order);
    if (tid < nbest) {
        const int q = tid;
        const int j = q < nb ? s_sel.order[q] : 0;
        const bool keep = q < nb && s_fin[j] > NEG_INF;
        write_hyp(b, q, nbest, T, keep, C.len[j], C.node[j], s_fin[j], s_spb[j], s_lmt[j], pool, T * K, out_labels, out_lens,
                  out_scores);
    }
}

}  // namespace

extern "C" size_t vocr_ctc_word_beam_workspace_bytes(int t, int b, int v, int beam, int nbest) {
    if (t <= 0 || b <= 0 || v <= 0 || v > VMAX || beam < 1 || beam > KMAX || nbest < 1 || nbest > beam) return 0;
    return (size_t)t * b * beam * sizeof(int2);
}

extern "C" int vocr_ctc_word_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam,
                                         int nbest, const int32_t* cls_kind, const int32_t* cls_tok, const int32_t* trie_next,
                                         const int32_t* trie_tok, const float* trie_la, int trie_nodes, const int32_t* lm_off,
                                         const int32_t* lm_succ_tok, const float* lm_succ_logp, const int32_t* lm_succ_next,
                                         const float* lm_bow, const int32_t* lm_back, int lm_states, int lm_succ, int lm_tokens,
                                         int lm_start, int tok_unk, int tok_eos, float lm_weight, float word_bonus, float oov_penalty,
                                         int32_t* out_labels, int32_t* out_lens, float* out_scores, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    VOCR_CHECK_ARG(cls_kind && cls_tok && trie_next && trie_tok && trie_la && lm_off && lm_succ_tok && lm_succ_logp && lm_succ_next &&
                       lm_bow && lm_back,
                   "vocr_ctc_word_beam_search: null table pointer");
    VOCR_CHECK_ARG(trie_nodes >= 1 && lm_states >= 1 && lm_tokens >= 1 && lm_succ >= lm_tokens,
                   "vocr_ctc_word_beam_search: need trie_nodes >= 1, lm_states >= 1, lm_tokens >= 1, lm_succ >= lm_tokens "
                   "(trie_nodes=%d lm_states=%d lm_tokens=%d lm_succ=%d)",
                   trie_nodes, lm_states, lm_tokens, lm_succ);
    VOCR_CHECK_ARG(lm_start >= 0 && lm_start < lm_states && tok_unk >= 0 && tok_unk < lm_tokens && tok_eos >= 0 && tok_eos < lm_tokens,
                   "vocr_ctc_word_beam_search: need 0 <= lm_start < lm_states and 0 <= tok_unk, tok_eos < lm_tokens (lm_start=%d "
                   "tok_unk=%d tok_eos=%d)",
                   lm_start, tok_unk, tok_eos);
    VOCR_CHECK_ARG((long)trie_nodes * v < (1L << 31), "vocr_ctc_word_beam_search: trie_nodes*v too large");
    VOCR_CHECK_ARG(__builtin_isfinite(lm_weight) && __builtin_isfinite(word_bonus) && !__builtin_isnan(oov_penalty) && oov_penalty < INFINITY,
                   "vocr_ctc_word_beam_search: lm_weight and word_bonus must be finite, oov_penalty finite or -inf");
    static VocrPerDevice lds_set;
    if (const int rc = check_search_args("vocr_ctc_word_beam_search", logits, lens, t, b, v, beam, nbest, out_labels, out_lens, out_scores,
                                         workspace, workspace_bytes, vocr_ctc_word_beam_workspace_bytes(t, b, v, beam, nbest),
                                         (const void*)ctc_word_beam_kernel, &lds_set))
        return rc;
    WordLm L;
    L.kind = cls_kind; L.tok = cls_tok; L.trie_next = trie_next; L.trie_tok = trie_tok; L.trie_la = trie_la;
    L.off = lm_off; L.succ_tok = lm_succ_tok; L.succ_logp = lm_succ_logp; L.succ_next = lm_succ_next; L.bow = lm_bow; L.back = lm_back;
    L.V = v; L.N = trie_nodes; L.S = lm_states; L.E = lm_succ; L.W = lm_tokens; L.start = lm_start; L.unk = tok_unk; L.eos = tok_eos;
    L.oov = oov_penalty;
    const size_t lds = (size_t)beam * v * sizeof(float);
    ctc_word_beam_kernel<<<b, BT, lds, (hipStream_t)stream>>>(logits, lens, t, b, v, canon, beam, nbest, L, lm_weight, word_bonus,
                                                              out_labels, out_lens, out_scores, (int2*)workspace);
    VOCR_CHECK_LAUNCH("vocr_ctc_word_beam_search");
    return VOCR_OK;
}
