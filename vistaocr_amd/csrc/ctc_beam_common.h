// Shared pieces of the CTC prefix beam searches: ctc_beam.hip (one kernel, instantiated without and with a grammar: the character
// n-gram search and the same search restricted to the labellings an automaton accepts) and ctc_word_beam.hip (word n-gram +
// lexicon).  One workgroup of BT threads per line; every device function here is called by all BT threads of the workgroup (the
// ones that synchronise say so) except stay_and_merge, which one thread per beam calls.  What the kernels share: the symbol classes
// and their per-frame log-probabilities, the stay probabilities with the exact merge of an extension into the beam that already
// holds its prefix, the radix top-K over the K*V candidate scores under the total order (score desc, slot id asc), the final ranking
// and the backtrack of the n-best from the node pool; on the host, the argument checks all three entries make.  Only integer LDS
// atomics; every float is computed by a fixed thread in a fixed order.
#pragma once
#include "ctc_math.h"

namespace ctcbeam {

constexpr int BT = 256;            // threads per line
constexpr int KMAX = 128;

// order-preserving map of a non-NaN float to uint32 (larger score -> larger key)
__device__ __forceinline__ unsigned score_key(float s) {
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long hash_push(unsigned long long h, int c) {
    return (h ^ (unsigned long long)(c + 1)) * 0x100000001b3ull + 0x9e3779b97f4a7c15ull;
}

constexpr unsigned long long HASH_ROOT = 0x84222325cbf29ce4ull;

// inclusive prefix sum over the 256 threads (every thread calls it)
__device__ __forceinline__ int block_scan(int v, int* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    int add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    __syncthreads();
    return v + add;
}

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return r;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

// Per-frame symbol classes: cls[v] the sanitised canonical index, chain[v] the next member of v's class; lp[c] the class
// log-probability (-inf on non-canonical columns), xp[c] the extension log-probability (lp, or -inf for the blank, pruned classes).
struct Frame {
    float lp[VMAX], xp[VMAX], row[VMAX];
    int cls[VMAX], chain[VMAX];
    float red[4];
};

// sanitised canon (class_of), member chains.  Ends with a barrier.
__device__ __forceinline__ void init_classes(const int32_t* __restrict__ canon, int V, Frame& f) {
    const int tid = threadIdx.x;
    if (tid < V) f.cls[tid] = class_of(canon, tid);
    __syncthreads();
    if (tid < V) {
        int nx = -1;
        for (int w = tid + 1; w < V; ++w)
            if (f.cls[w] == f.cls[tid]) { nx = w; break; }
        f.chain[tid] = nx;
    }
    __syncthreads();
}

// row log-softmax of the raw logits of one frame, then the class log-probs.  Ends with a barrier.
__device__ __forceinline__ void frame_logprobs(const float* __restrict__ row, int V, float prune, Frame& f) {
    const int tid = threadIdx.x;
    const float x = tid < V ? row[tid] : NEG_INF;
    const float m = block_max(x, f.red);
    const float se = block_sum(tid < V && m != NEG_INF ? expf(x - m) : 0.f, f.red);
    const float lse = m + logf(se);
    if (tid < V) f.row[tid] = x - lse;
    __syncthreads();
    if (tid < V) {
        float lp = NEG_INF;
        if (f.cls[tid] == tid) {
            float mm = NEG_INF;
            for (int v = tid; v >= 0; v = f.chain[v]) mm = fmaxf(mm, f.row[v]);
            if (f.chain[tid] < 0) {
                lp = f.row[tid];
            } else if (mm != NEG_INF) {
                float ss = 0.f;
                for (int v = tid; v >= 0; v = f.chain[v]) ss += expf(f.row[v] - mm);
                lp = mm + logf(ss);
            }
        }
        f.lp[tid] = lp;
        f.xp[tid] = (tid > 0 && lp > NEG_INF && lp >= prune) ? lp : NEG_INF;
    }
    __syncthreads();
}

// The beam k < nb that holds the parent prefix of beam j (-1: none), for j's merge.  Identity of prefixes is exact: a 64-bit
// rolling hash plus the length filter, and every hash match is confirmed by walking both node chains in the pool until they meet
// at one node (same node => same rest of the prefix) or a class differs.  Pool indices outside [0, npool) end the walk.
__device__ __forceinline__ int find_merge(int j, int nb, const int* len, const int* last, const int* node,
                                          const unsigned long long* hash, const unsigned long long* phash, const float* xp,
                                          const int2* __restrict__ pool, int npool) {
    const int lj = len[j], cj = last[j];
    int mk = -1;
    if (lj > 0 && xp[cj] > NEG_INF) {
        const int pj = (node[j] >= 0 && node[j] < npool) ? pool[node[j]].x : -1;
        for (int k = 0; k < nb && mk < 0; ++k) {
            if (len[k] != lj - 1 || hash[k] != phash[j]) continue;
            int a = node[k], p = pj;
            bool same = true;
            while (a != p) {                  // equal lengths: both chains reach the root (-1) together
                if (a < 0 || p < 0 || a >= npool || p >= npool) { same = false; break; }
                const int2 na = pool[a], np = pool[p];
                if (na.y != np.y) { same = false; break; }
                a = na.x; p = np.x;
            }
            if (same) mk = k;
        }
    }
    return mk;
}

// Step 2 of the frame loop, by thread j < nb: the "stay" probabilities of beam j (spb: after a blank, spnb: after a repeat of its
// last class, with the extension merged in that re-creates prefix j from the beam merge[j] holding its parent prefix).  Buf is a
// kernel's beam buffer (pb, pnb, last, len, node, hash, phash); the caller synchronises.
template <class Buf>
__device__ __forceinline__ void stay_and_merge(const Buf& C, int j, int nb, const Frame& f, const int2* __restrict__ pool, int npool,
                                               int* merge, float* spb, float* spnb) {
    const int lj = C.len[j], cj = C.last[j];
    const int mk = find_merge(j, nb, C.len, C.last, C.node, C.hash, C.phash, f.xp, pool, npool);
    merge[j] = mk;
    const float pbj = C.pb[j], pnbj = C.pnb[j];
    float s = lj > 0 ? pnbj + f.lp[cj] : NEG_INF;
    if (mk >= 0) {
        const float base = (cj == C.last[mk]) ? C.pb[mk] : lse2(C.pb[mk], C.pnb[mk]);
        s = lse2(s, base + f.xp[cj]);
    }
    spb[j] = lse2(pbj, pnbj) + f.lp[0];
    spnb[j] = s;
}

struct Select {
    int selid[KMAX], order[KMAX];
    unsigned selkey[KMAX];
    int hist[256];
    int wsum[4];
    int bin, before, eqcnt, total, nsel;
};

// The top K of the ncand scores in LDS under (score desc, id asc), -inf never taken: radix select over the fp32 bits (4 passes
// of 8 bits), two more passes over the ids where several candidates share the K-th score, then ranking by counting (K^2 compares).
// Returns the number kept; sel.order[0..n) holds their ids in rank order.  The caller has synchronised after writing the scores;
// ends with a barrier.
__device__ __forceinline__ int top_k(const float* __restrict__ s_score, int ncand, int K, Select& sel) {
    const int tid = threadIdx.x;
    if (tid == 0) sel.nsel = 0;
    unsigned prefix = 0, mask = 0;
    int need = K;
    bool take_all = false;
    for (int shift = 24; shift >= 0; shift -= 8) {
        sel.hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < ncand; i += BT) {
            const float sc = s_score[i];
            if (!(sc > NEG_INF)) continue;
            const unsigned u = score_key(sc);
            if ((u & mask) == prefix) atomicAdd(&sel.hist[(u >> shift) & 255], 1);
        }
        __syncthreads();
        const int cnt = sel.hist[255 - tid];
        const int incl = block_scan(cnt, sel.wsum);
        if (shift == 24 && tid == BT - 1) sel.total = incl;
        if (incl >= need && incl - cnt < need) { sel.bin = 255 - tid; sel.before = incl - cnt; sel.eqcnt = cnt; }
        __syncthreads();
        if (shift == 24 && sel.total <= K) { take_all = true; break; }
        need -= sel.before;
        prefix |= (unsigned)sel.bin << shift;
        mask |= 255u << shift;
        __syncthreads();                              // bin / before are rewritten by the next pass
    }
    int id_cut = 0x7fffffff;
    if (!take_all && sel.eqcnt > need) {              // ties at the K-th score: the smallest ids among them
        int idp = 0, idm = 0;
        for (int shift = 8; shift >= 0; shift -= 8) {
            sel.hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < ncand; i += BT) {
                const float sc = s_score[i];
                if (!(sc > NEG_INF) || score_key(sc) != prefix || (i & idm) != idp) continue;
                atomicAdd(&sel.hist[(i >> shift) & 255], 1);
            }
            __syncthreads();
            const int cnt = sel.hist[tid];
            const int incl = block_scan(cnt, sel.wsum);
            if (incl >= need && incl - cnt < need) { sel.bin = tid; sel.before = incl - cnt; }
            __syncthreads();
            need -= sel.before;
            idp |= sel.bin << shift;
            idm |= 255 << shift;
            __syncthreads();
        }
        id_cut = idp;
    }
    for (int i = tid; i < ncand; i += BT) {
        const float sc = s_score[i];
        if (!(sc > NEG_INF)) continue;
        const unsigned u = score_key(sc);
        if (take_all || u > prefix || (u == prefix && i <= id_cut)) {
            const int slot = atomicAdd(&sel.nsel, 1);
            if (slot < KMAX) { sel.selid[slot] = i; sel.selkey[slot] = u; }
        }
    }
    __syncthreads();
    const int nsel = min(sel.nsel, K);
    if (tid < nsel) {
        const unsigned u = sel.selkey[tid];
        const int id = sel.selid[tid];
        int r = 0;
        for (int q = 0; q < nsel; ++q) {
            const unsigned uq = sel.selkey[q];
            r += (uq > u || (uq == u && sel.selid[q] < id)) ? 1 : 0;
        }
        sel.order[r] = id;
    }
    __syncthreads();
    return nsel;
}

// End of line: order[r] = the beam of rank r by the final scores f[0..nb) (ties: the rank at the last frame; NaN ranks last).
// Ends with a barrier.
__device__ __forceinline__ void rank_final(const float* f, int nb, int* order) {
    const int tid = threadIdx.x;
    if (tid < nb) {
        const float v = f[tid];
        const unsigned u = v == v ? score_key(v) : 0u;
        int r = 0;
        for (int q = 0; q < nb; ++q) {
            const float fq = f[q];
            const unsigned uq = fq == fq ? score_key(fq) : 0u;
            r += (uq > u || (uq == u && q < tid)) ? 1 : 0;
        }
        order[r] = tid;
    }
    __syncthreads();
}

// Output rank q of line b: the labelling of length n ending at pool node `node` with scores s0..s2, or (keep = false) an empty
// rank: length 0, total and acoustic -inf, LM 0.  Labels past the length are zero.
__device__ __forceinline__ void write_hyp(int b, int q, int nbest, int T, bool keep, int n, int node, float s0, float s1, float s2,
                                          const int2* __restrict__ pool, int npool, int32_t* __restrict__ out_labels,
                                          int32_t* __restrict__ out_lens, float* __restrict__ out_scores) {
    int32_t* lab = out_labels + ((long)b * nbest + q) * T;
    float* sc = out_scores + ((long)b * nbest + q) * 3;
    if (keep) {
        n = min(n, T);
        for (int p = n - 1; p >= 0; --p) {
            int2 nd = (node >= 0 && node < npool) ? pool[node] : make_int2(-1, 0);
            lab[p] = nd.y;
            node = nd.x;
        }
        sc[0] = s0; sc[1] = s1; sc[2] = s2;
    } else {
        n = 0;
        sc[0] = NEG_INF; sc[1] = NEG_INF; sc[2] = 0.f;
    }
    for (int p = n; p < T; ++p) lab[p] = 0;
    out_lens[(long)b * nbest + q] = n;
}

// Host: what every search entry checks under its own name `who` once its own arguments have passed - the pointers, the shape, the
// beam, the pool's index range, the workspace against `need` (the entry's own *_workspace_bytes) - and the opt-in of `kernel` to
// KMAX * VMAX candidate scores of dynamic LDS (`lds_set`: the entry's own static flags).  VOCR_OK, or the error to return.
inline int check_search_args(const char* who, const void* logits, const void* lens, int t, int b, int v, int beam, int nbest,
                             const void* out_labels, const void* out_lens, const void* out_scores, const void* workspace,
                             size_t workspace_bytes, size_t need, const void* kernel, VocrPerDevice* lds_set) {
    VOCR_CHECK_ARG(logits && lens && out_labels && out_lens && out_scores && workspace, "%s: null pointer", who);
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 0 && v <= VMAX, "%s: need t > 0, b > 0, 1 <= v <= %d (t=%d b=%d v=%d)", who, VMAX, t, b, v);
    VOCR_CHECK_ARG(beam >= 1 && beam <= KMAX, "%s: need 1 <= beam <= %d (beam=%d)", who, KMAX, beam);
    VOCR_CHECK_ARG(nbest >= 1 && nbest <= beam, "%s: need 1 <= nbest <= beam (nbest=%d beam=%d)", who, nbest, beam);
    VOCR_CHECK_ARG((long)t * b * beam < (1L << 31) && (long)t * beam < (1L << 30), "%s: t*b*beam too large", who);
    VOCR_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    return vocr_allow_dynamic_lds(&kernel, 1, KMAX * VMAX * (int)sizeof(float), lds_set, who);
}

}  // namespace ctcbeam
