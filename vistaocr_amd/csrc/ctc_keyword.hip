// CTC keyword search: for every (line, query) the EXPECTED NUMBER of occurrences of the query as a contiguous substring of the collapsed
// labelling, E = sum over all frame paths pi of P(pi | x) * #occurrences(query in B(pi)), and the best single occurrence with its frame
// span.  Exact under the CTC model (a sum over all V^len paths, no beam, no hypothesis, no pruning) because the frames are independent
// given the input: one forward recursion per (line, query).  Conventions are vocr_ctc_align's: blank = 0, classes from canon[V], the
// skip s-2 -> s iff position s is a label whose CLASS differs from that of s-2.
//
// A query k_1 .. k_L has S = 2L-1 extended positions k_1, blank, k_2, .., blank, k_L (no outer blanks).  An occurrence is a MAXIMAL
// frame span [s, e]: pi_s in k_1's class, pi_e in k_L's, pi_s .. pi_e collapses to the query, pi_(s-1) not in k_1's class (or s = 0),
// pi_(e+1) not in k_L's class (or e = len-1).  With notc_t(c) = ln(1 - P_t(class of c)):
//   entry(t) = 0 if t = 0 else notc_(t-1)(k_1)        ANCHOR_START: sum of ln p_u(blank) over u < t
//   exit(t)  = 0 if t = len-1 else notc_(t+1)(k_L)    ANCHOR_END:   sum of ln p_u(blank) over u > t
//   a_t(0)   = lp_t(k_1) + lse(a_(t-1)(0), entry(t))
//   a_t(s)   = lp_t(ext_s) + lse(a_(t-1)(s), a_(t-1)(s-1), a_(t-1)(s-2) if the skip is allowed)
//   ln E     = lse over t of a_t(S-1) + exit(t)
// and the same recursion with max for the best occurrence, every cell carrying the start frame of its best path (no back pointers).
// TIE RULE: among equal candidates prefer s (stay), then s-1, then s-2, then the fresh entry (position 0 only: it takes the s-1 slot
// there); a candidate replaces the choice only when STRICTLY greater; among equal end frames the earliest wins.
//
//   kernel 1  class log-probabilities : class_logprob_rows_kernel of the alignment.
//   kernel 2  not-class rows          : one wave per (t, b) row: notc[row][v] = ln of the SUM of the other classes' probabilities, as
//                                       (max of the others - row max) + (ln sum of their exponentials - ln row sum); never 1 - p, which
//                                       cancels at every peak of a trained net.  The row and its exponentials sit in LDS; column v sums
//                                       the columns of the other classes in index order, four interleaved partial sums.
//   kernel 3  blank sums              : one wave per line: exclusive prefix and suffix sums of ln p_t(blank), by 64-frame shuffle scans.
//   kernel 4  plan                    : one workgroup validates the queries and sorts them (stable counting sort) by lane layout:
//                                       S <= 16, S <= 32, S <= 64 (one position per lane; 4 / 2 / 1 queries per wave in lane segments)
//                                       and S <= 256 (four positions per lane).  The queries live in device memory, so the permutation
//                                       is made there; nothing is copied to the host.
//   kernel 5  search                  : one wave per (line, group of queries of one layout); neighbours by (segment-wide) shuffles, the
//                                       gathered lp_t(ext_s) and the two boundary scalars prefetched PF frames ahead.  The grid is sized
//                                       for the worst case (no two queries share a wave); waves beyond the plan's count leave at once.
// Every float is computed by a fixed lane in a fixed order and the only cross-lane operations are shuffles and ballots: results are
// bit-identical from run to run.  No LDS and no barrier in the search.
#include "ctc_align_common.h"

namespace {

constexpr int QLEN_MAX = 128;                // S = 255 positions: four per lane
constexpr int ANCHOR_START = 1, ANCHOR_END = 2;
constexpr int TRIM_START = 4, TRIM_END = 8;     // the span leaves out the first / last label (whole-word search pads with spaces)
constexpr int NLAYOUT = 4;                   // S <= 16, <= 32, <= 64, <= 256

// 16 rows per block, one wave per row at a time.  notc[row][v] = ln(1 - P(class of v | frame)) from the raw logits; rows with
// t >= lens[b] are never read and not written.  A row of -inf gives -inf.
__global__ __launch_bounds__(256) void not_class_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ canon, float* __restrict__ notc, int T, int B,
                                                             int V) {
    __shared__ int s_cls[VMAX];
    __shared__ float s_row[4][VMAX];
    __shared__ float s_exp[4][VMAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < V) s_cls[tid] = class_of(canon, tid);
    __syncthreads();
    float* rw = s_row[wave];
    float* ew = s_exp[wave];
    for (int r = wave; r < ROWS_PER_BLOCK; r += 4) {
        const int row = blockIdx.x * ROWS_PER_BLOCK + r;
        if (row >= T * B) break;
        const int t = row / B, b = row - t * B;
        if (t >= min(max(lens[b], 0), T)) continue;
        const float* xr = x + (long)row * V;
        float* out = notc + (long)row * V;
        __builtin_amdgcn_wave_barrier();                          // the previous row's readers are done with rw / ew
        float m = NEG_INF;
        for (int v = lane; v < V; v += 64) {
            const float xv = xr[v];
            rw[v] = xv;
            m = fmaxf(m, xv);
        }
        m = wave_max(m);
        if (m == NEG_INF) {
            for (int v = lane; v < V; v += 64) out[v] = NEG_INF;
            continue;
        }
        __builtin_amdgcn_wave_barrier();
        // cm: the class of the first column that holds the row's maximum; m2: the maximum over the columns of every other class
        int first = VMAX;
        for (int v = lane; v < V; v += 64)
            if (rw[v] == m) first = min(first, v);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        const int cm = s_cls[min(first, V - 1)];                  // (a NaN row matches nothing)
        float m2 = NEG_INF, s = 0.f;
        for (int v = lane; v < V; v += 64) {
            const float e = expf(rw[v] - m);
            ew[v] = e;
            s += e;
            if (s_cls[v] != cm) m2 = fmaxf(m2, rw[v]);
        }
        s = wave_sum(s);
        m2 = wave_max(m2);
        float s2 = 0.f;                                           // the other classes' sum for the columns of class cm, relative to m2
        if (m2 != NEG_INF)
            for (int v = lane; v < V; v += 64)
                if (s_cls[v] != cm) s2 += expf(rw[v] - m2);
        s2 = wave_sum(s2);
        const float ls = logf(s);
        const float n_cm = m2 == NEG_INF ? NEG_INF : (m2 - m) + (logf(s2) - ls);
        __builtin_amdgcn_wave_barrier();
        for (int v = lane; v < V; v += 64) {
            const int c = s_cls[v];
            float r_ = n_cm;
            if (c != cm) {                                        // the maximum is among the others: their sum relative to m
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                int w = 0;
                for (; w + 4 <= V; w += 4) {
                    a0 += s_cls[w] != c ? ew[w] : 0.f;
                    a1 += s_cls[w + 1] != c ? ew[w + 1] : 0.f;
                    a2 += s_cls[w + 2] != c ? ew[w + 2] : 0.f;
                    a3 += s_cls[w + 3] != c ? ew[w + 3] : 0.f;
                }
                for (; w < V; ++w) a0 += s_cls[w] != c ? ew[w] : 0.f;
                r_ = logf((a0 + a1) + (a2 + a3)) - ls;
            }
            out[v] = r_;
        }
    }
}

// grid.x = B, 64 threads.  pre[b][t] = sum of clp[u][b][0] over u < t, suf[b][t] = the sum over t < u < len, for t < len.
__global__ __launch_bounds__(64) void blank_sums_kernel(const float* __restrict__ clp, const int32_t* __restrict__ lens, int T, int B, int V,
                                                        float* __restrict__ pre, float* __restrict__ suf) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int len = min(max(lens[b], 0), T);
    const long tstride = (long)B * V;
    const float* col = clp + (long)b * V;
    for (int dir = 0; dir < 2; ++dir) {
        float* dst = (dir ? suf : pre) + (long)b * T;
        float carry = 0.f;
        for (int t0 = 0; t0 < len; t0 += 64) {
            const int i = t0 + lane;                              // the i-th frame from this direction's end
            const int t = dir ? len - 1 - i : i;
            float v = i < len ? col[(long)t * tstride] : 0.f;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float u = __shfl_up(v, o, 64);
                if (lane >= o) v += u;
            }
            float ex = __shfl_up(v, 1, 64);                       // exclusive: no subtraction (-inf - -inf)
            if (lane == 0) ex = 0.f;
            if (i < len) dst[t] = carry + ex;
            carry += __shfl(v, 63, 64);
        }
    }
}

// the plan in front of the workspace's integer part: hdr[0..3] the number of queries of each layout, hdr[4..7] where each layout's
// queries start in perm, hdr[8..11] where each layout's waves start in a line's wave list, hdr[12] the waves of one line
constexpr int HDR = 16;

__device__ __forceinline__ int layout_of(int S, int pack) {
    if (S > 64) return 3;
    if (!pack || S > 32) return 2;
    return S > 16 ? 1 : 0;
}


// one workgroup of 256 threads.  perm[i] = query index | bad << 31, sorted by layout, stable; key[nq] is scratch.  An invalid query
// (length outside [1, max_query_len], a label <= 0 or >= V or in the blank's class, fewer labels than a trimmed span needs) takes a
// slot of the narrowest layout and is marked.
__global__ __launch_bounds__(256) void keyword_plan_kernel(const int32_t* __restrict__ canon, const int32_t* __restrict__ queries,
                                                           const int32_t* __restrict__ query_lens,
                                                           const int32_t* __restrict__ query_flags, int V, int nq, int query_stride,
                                                           int max_query_len, int pack, int32_t* __restrict__ hdr,
                                                           int32_t* __restrict__ perm, int32_t* __restrict__ key) {
    __shared__ int s_cnt[NLAYOUT][256];
    __shared__ int s_tot[NLAYOUT];
    const int tid = threadIdx.x;
    const int per = (nq + 255) / 256;
    const int q0 = (int)min((long)tid * per, (long)nq), q1 = (int)min((long)q0 + per, (long)nq);
    int cnt[NLAYOUT] = {0, 0, 0, 0};
    for (int q = q0; q < q1; ++q) {
        const int L = query_lens[q];
        const int fl = query_flags ? query_flags[q] : 0;
        const int trims = ((fl & TRIM_START) ? 1 : 0) + ((fl & TRIM_END) ? 1 : 0);
        bool bad = L < 1 || L > max_query_len || L < 1 + trims;  // a trimmed span keeps at least one label
        if (!bad) {
            const int32_t* lab = queries + (long)q * query_stride;
            for (int p = 0; p < L; ++p) {
                const int v = lab[p];
                bad |= (v <= 0 || v >= V) || class_of(canon, min(max(v, 0), V - 1)) == 0;
            }
        }
        const int k = bad ? layout_of(1, pack) : layout_of(2 * L - 1, pack);
        key[q] = k | (bad ? 4 : 0);
#pragma unroll
        for (int j = 0; j < NLAYOUT; ++j) cnt[j] += k == j ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < NLAYOUT; ++k) s_cnt[k][tid] = cnt[k];
    __syncthreads();
    if (tid < NLAYOUT) {                                          // exclusive scan over the threads, serial: 256 adds
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int c = s_cnt[tid][i];
            s_cnt[tid][i] = run;
            run += c;
        }
        s_tot[tid] = run;
    }
    __syncthreads();
    int off[NLAYOUT], run = 0;
#pragma unroll
    for (int k = 0; k < NLAYOUT; ++k) {
        off[k] = run + s_cnt[k][tid];
        run += s_tot[k];
    }
    if (tid == 0) {
        int waves = 0, qb = 0;
        for (int k = 0; k < NLAYOUT; ++k) {
            hdr[k] = s_tot[k];
            hdr[4 + k] = qb;
            qb += s_tot[k];
        }
        for (int k = NLAYOUT - 1; k >= 0; --k) {                  // the longest queries first
            hdr[8 + k] = waves;
            const int per_wave = k == 0 ? 4 : k == 1 ? 2 : 1;
            waves += (s_tot[k] + per_wave - 1) / per_wave;
        }
        hdr[12] = waves;
    }
    for (int q = q0; q < q1; ++q) {
        const int kk = key[q], k = kk & 3;
        int o = 0;
#pragma unroll
        for (int j = 0; j < NLAYOUT; ++j)
            if (k == j) o = off[j]++;
        perm[o] = q | ((kk & 4) ? (int)0x80000000 : 0);
    }
}

// one cell of both recursions: the expected-count value a and the best path's (score m, start frame ms) from the cell itself, its
// s-1 slot and its s-2 slot (-inf where there is none), in the tie rule's order
struct Cell {
    float a, m;
    int ms, me;            // me: the last frame the best path spent on the label before the last one (TRIM_END)
};

// restart: the cell of the second label under TRIM_START (a path that arrives there starts its span now); mark: the cell of the label
// before the last one (it is the span's end for as long as the path stays)
__device__ __forceinline__ Cell cell_step(const Cell& self, float a1, float m1, int s1, int e1, float a2, float m2, int s2, int e2,
                                          float lpe, bool in, bool restart, bool mark, int t) {
    Cell r;
    float best = self.m;
    r.ms = self.ms;
    r.me = self.me;
    if (m1 > best) { best = m1; r.ms = restart ? t : s1; r.me = e1; }
    if (m2 > best) { best = m2; r.ms = restart ? t : s2; r.me = e2; }
    if (mark) r.me = t;
    const float l = lse3(self.a, a1, a2);
    r.a = in ? l + lpe : NEG_INF;
    r.m = in ? best + lpe : NEG_INF;
    return r;
}

// One wave, 64 / SEG queries of line b in lane segments of SEG lanes, NP positions per lane (NP = 1, or NP = 4 with SEG = 64: position
// 4 * lane + j, so j = 0, 2 are labels and j = 1, 3 blanks).  perm_k / n_k: the layout's slice of the plan; item: which group of it.
template <int SEG, int NP, int PF>
__device__ __forceinline__ void keyword_wave(const float* __restrict__ clp, const float* __restrict__ notc, const float* __restrict__ pre,
                                             const float* __restrict__ suf, const int32_t* __restrict__ canon,
                                             const int32_t* __restrict__ queries, const int32_t* __restrict__ query_lens,
                                             const int32_t* __restrict__ query_flags, int T, int B, int V, int nq, int query_stride, int b,
                                             int len, const int32_t* __restrict__ perm_k, int n_k, int item,
                                             float* __restrict__ out_log_count, float* __restrict__ out_best, int32_t* __restrict__ out_span) {
    static_assert(NP == 1 || (NP == 4 && SEG == 64), "layouts");
    constexpr int NL = NP == 1 ? 1 : 2;                            // label positions per lane
    const int lane = threadIdx.x & 63, seg = lane / SEG, sl = lane % SEG;
    const int idx = item * (64 / SEG) + seg;
    const bool has = idx < n_k;
    const int pe = has ? perm_k[idx] : (int)0x80000000;
    const int q = pe & 0x7fffffff;
    const bool run = pe >= 0 && len > 0;
    const int L = run ? query_lens[q] : 1;
    const int S = 2 * L - 1;
    const int32_t* lab = queries + (long)q * query_stride;
    const int flags = (run && query_flags) ? query_flags[q] : 0;
    const long tstride = (long)B * V;
    const float* lpb = clp + (long)b * V;

    // the lane's label positions: s = sl (NP = 1, labels on even s) or 4 * sl and 4 * sl + 2
    int e[NL], c[NL];
    bool in[NL], skip[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int s = NP == 1 ? sl : 4 * sl + 2 * j;
        in[j] = run && s < S;
        e[j] = (in[j] && !(s & 1)) ? lab[s >> 1] : 0;
        c[j] = class_of(canon, e[j]);
    }
    if (NP == 1) {
        const int c_m2 = __shfl_up(c[0], 2, SEG);
        skip[0] = in[0] && sl >= 2 && !(sl & 1) && c[0] != c_m2;
    } else {
        const int c_m2 = __shfl_up(c[NL - 1], 1, SEG);
        skip[0] = in[0] && sl >= 1 && c[0] != c_m2;
        skip[NL - 1] = in[NL - 1] && c[NL - 1] != c[0];
    }
    const bool in_b1 = NP == 4 && run && 4 * sl + 1 < S, in_b3 = NP == 4 && run && 4 * sl + 3 < S;
    // the label positions where a trimmed span starts (s = 2) and ends (s = S-3)
    bool restart[NL], mark[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int s = NP == 1 ? sl : 4 * sl + 2 * j;
        restart[j] = (flags & TRIM_START) && s == 2;
        mark[j] = (flags & TRIM_END) && s == S - 3;
    }
    const bool trim_end = __any(flags & TRIM_END);                 // wave-uniform: the end frame travels by shuffles only where needed
    const int k1 = run ? lab[0] : 0, kL = run ? lab[L - 1] : 0;
    const bool a_start = flags & ANCHOR_START, a_end = flags & ANCHOR_END;
    const float* en_base = a_start ? pre + (long)b * T : notc + (long)b * V + k1;
    const float* ex_base = a_end ? suf + (long)b * T : notc + (long)b * V + kL;
    const long en_mul = a_start ? 1 : tstride, ex_mul = a_end ? 1 : tstride;
    const int en_shift = a_start ? 0 : 1, ex_shift = a_end ? 0 : 1;

    struct Frame {
        float lp[NL], lp0, en, ex;
    };
    auto load = [&](int t) {
        Frame f;
        t = min(t, len - 1);
#pragma unroll
        for (int j = 0; j < NL; ++j) f.lp[j] = lpb[t * tstride + e[j]];
        f.lp0 = NP == 4 ? lpb[t * tstride] : 0.f;
        f.en = en_base[max(t - en_shift, 0) * en_mul];
        f.ex = ex_base[min(t + ex_shift, len - 1) * ex_mul];
        return f;
    };

    constexpr int NC = NP == 1 ? 1 : 4;
    Cell cell[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) cell[j] = {NEG_INF, NEG_INF, -1, -1};
    LseAcc acc;
    float best = NEG_INF;
    int best_s = -1, best_e = -1;
    const int fin_lane = (S - 1) / NP;
    const bool fin_hi = NP == 4 && ((S - 1) & 2);                  // the last label is the lane's second one

    if (len > 0) {                                                 // wave-uniform
        Frame buf[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) buf[k] = load(k);
        for (int t0 = 0; t0 < len; t0 += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const int t = t0 + k;
                if (t < len) {                                     // wave-uniform
                    const Frame f = buf[k];
                    buf[k] = load(t + PF);
                    const float en = (t == 0 && !a_start) ? 0.f : f.en;
                    const float ex = (t == len - 1 && !a_end) ? 0.f : f.ex;
                    Cell fin;
                    if (NP == 1) {
                        float a1 = __shfl_up(cell[0].a, 1, SEG), a2 = __shfl_up(cell[0].a, 2, SEG);
                        float m1 = __shfl_up(cell[0].m, 1, SEG), m2 = __shfl_up(cell[0].m, 2, SEG);
                        int s1 = __shfl_up(cell[0].ms, 1, SEG), s2 = __shfl_up(cell[0].ms, 2, SEG);
                        int e1 = -1, e2 = -1;
                        if (trim_end) { e1 = __shfl_up(cell[0].me, 1, SEG); e2 = __shfl_up(cell[0].me, 2, SEG); }
                        if (sl == 0) { a1 = en; m1 = en; s1 = t; }          // the fresh entry takes the s-1 slot of position 0
                        if (!skip[0]) { a2 = NEG_INF; m2 = NEG_INF; }
                        cell[0] = cell_step(cell[0], a1, m1, s1, e1, a2, m2, s2, e2, f.lp[0], in[0], restart[0], mark[0], t);
                        fin = cell[0];
                    } else {
                        float a3 = __shfl_up(cell[3].a, 1, SEG), a2 = __shfl_up(cell[2].a, 1, SEG);
                        float m3 = __shfl_up(cell[3].m, 1, SEG), m2 = __shfl_up(cell[2].m, 1, SEG);
                        int s3 = __shfl_up(cell[3].ms, 1, SEG), s2 = __shfl_up(cell[2].ms, 1, SEG);
                        int e3 = -1, e2 = -1;
                        if (trim_end) { e3 = __shfl_up(cell[3].me, 1, SEG); e2 = __shfl_up(cell[2].me, 1, SEG); }
                        if (sl == 0) { a3 = en; m3 = en; s3 = t; }
                        if (!skip[0]) { a2 = NEG_INF; m2 = NEG_INF; }
                        const Cell o0 = cell[0], o1 = cell[1], o2 = cell[2];
                        cell[0] = cell_step(o0, a3, m3, s3, e3, a2, m2, s2, e2, f.lp[0], in[0], restart[0], mark[0], t);
                        cell[1] = cell_step(o1, o0.a, o0.m, o0.ms, o0.me, NEG_INF, NEG_INF, -1, -1, f.lp0, in_b1, false, false, t);
                        cell[2] = cell_step(o2, o1.a, o1.m, o1.ms, o1.me, skip[NL - 1] ? o0.a : NEG_INF, skip[NL - 1] ? o0.m : NEG_INF,
                                            o0.ms, o0.me, f.lp[NL - 1], in[NL - 1], restart[NL - 1], mark[NL - 1], t);
                        cell[3] = cell_step(cell[3], o2.a, o2.m, o2.ms, o2.me, NEG_INF, NEG_INF, -1, -1, f.lp0, in_b3, false, false, t);
                        fin = fin_hi ? cell[2] : cell[0];
                    }
                    // the last position (read on its own lane only): close an occurrence at t
                    acc.add(fin.a + ex);
                    const float mv = fin.m + ex;
                    if (mv > best) { best = mv; best_s = fin.ms; best_e = (flags & TRIM_END) ? fin.me : t; }
                }
            }
        }
    }
    if (has && sl == fin_lane) {
        const long o = (long)b * nq + q;
        const float lc = acc.get();
        out_log_count[o] = lc;
        out_best[o] = best;
        out_span[2 * o] = best == NEG_INF ? -1 : best_s;
        out_span[2 * o + 1] = best == NEG_INF ? -1 : best_e;
    }
}

// grid.x = ceil(B * nq / 4), 256 threads: wave w of the grid is (line w / hdr[12], wave w % hdr[12] of the line's wave list).
__global__ __launch_bounds__(256) void keyword_search_kernel(const float* __restrict__ clp, const float* __restrict__ notc,
                                                             const float* __restrict__ pre, const float* __restrict__ suf,
                                                             const int32_t* __restrict__ lens, const int32_t* __restrict__ canon,
                                                             const int32_t* __restrict__ queries, const int32_t* __restrict__ query_lens,
                                                             const int32_t* __restrict__ query_flags, int T, int B, int V, int nq,
                                                             int query_stride, const int32_t* __restrict__ hdr,
                                                             const int32_t* __restrict__ perm, float* __restrict__ out_log_count,
                                                             float* __restrict__ out_best, int32_t* __restrict__ out_span) {
    const long w = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = hdr[12];
    if (nw <= 0 || w >= (long)B * nw) return;
    const int b = (int)(w / nw);
    int item = (int)(w - (long)b * nw);
    const int k = item >= hdr[8] ? 0 : item >= hdr[9] ? 1 : item >= hdr[10] ? 2 : 3;
    item -= hdr[8 + k];
    const int len = min(max(lens[b], 0), T);
    const int32_t* pk = perm + hdr[4 + k];
    const int n_k = hdr[k];
#define KW_ARGS clp, notc, pre, suf, canon, queries, query_lens, query_flags, T, B, V, nq, query_stride, b, len, pk, n_k, item, \
                out_log_count, out_best, out_span
    if (k == 0) keyword_wave<16, 1, 8>(KW_ARGS);
    else if (k == 1) keyword_wave<32, 1, 8>(KW_ARGS);
    else if (k == 2) keyword_wave<64, 1, 8>(KW_ARGS);
    else keyword_wave<64, 4, 4>(KW_ARGS);
#undef KW_ARGS
}

struct Plan {
    size_t rows_bytes;     // one [T * B][V] fp32 matrix: the class log-probabilities, and again the not-class rows
    size_t sums_bytes;     // one [B][T] fp32 matrix: the blank prefix sums, and again the suffix sums
    size_t ints_bytes;     // the plan's header, the permutation and the sort's keys
    bool ok;
};

Plan plan_for(int t, int b, int v, int nq, int max_query_len) {
    Plan p = {0, 0, 0, false};
    if (t <= 0 || b <= 0 || v <= 1 || v > VMAX || nq < 1 || max_query_len < 1 || max_query_len > QLEN_MAX) return p;
    if ((long)t * b * nq >= (1L << 31)) return p;
    p.rows_bytes = clp_bytes(t, b, v);
    p.sums_bytes = align16((size_t)t * b * sizeof(float));
    p.ints_bytes = align16((size_t)(HDR + 2 * (size_t)nq) * sizeof(int32_t));
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t vocr_ctc_keyword_workspace_bytes(int t, int b, int v, int nq, int max_query_len) {
    const Plan p = plan_for(t, b, v, nq, max_query_len);
    if (!p.ok) return 0;
    return 2 * p.rows_bytes + 2 * p.sums_bytes + p.ints_bytes;
}

extern "C" int vocr_ctc_keyword_scores(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                       const int32_t* queries, const int32_t* query_lens, const int32_t* query_flags, int nq,
                                       int query_stride, int max_query_len, float* out_log_count, float* out_best, int32_t* out_span,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 1 && v <= VMAX, "vocr_ctc_keyword_scores: need t > 0, b > 0, 2 <= v <= %d (t=%d b=%d v=%d)", VMAX,
                   t, b, v);
    VOCR_CHECK_ARG(nq >= 1, "vocr_ctc_keyword_scores: need nq >= 1 (nq=%d)", nq);
    VOCR_CHECK_ARG(max_query_len >= 1 && max_query_len <= QLEN_MAX && query_stride >= max_query_len,
                   "vocr_ctc_keyword_scores: need 1 <= max_query_len <= %d and query_stride >= max_query_len (max_query_len=%d "
                   "query_stride=%d)", QLEN_MAX, max_query_len, query_stride);
    const Plan p = plan_for(t, b, v, nq, max_query_len);
    VOCR_CHECK_ARG(p.ok, "vocr_ctc_keyword_scores: unsupported shape (t=%d b=%d v=%d nq=%d max_query_len=%d): t*b*nq must stay below 2^31",
                   t, b, v, nq, max_query_len);
    VOCR_CHECK_ARG(logits && lens && queries && query_lens && out_log_count && out_best && out_span && workspace,
                   "vocr_ctc_keyword_scores: null pointer");
    const size_t need = vocr_ctc_keyword_workspace_bytes(t, b, v, nq, max_query_len);
    VOCR_CHECK_ARG(workspace_bytes >= need, "vocr_ctc_keyword_scores: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* clp = (float*)ws;
    float* notc = (float*)(ws + p.rows_bytes);
    float* pre = (float*)(ws + 2 * p.rows_bytes);
    float* suf = (float*)(ws + 2 * p.rows_bytes + p.sums_bytes);
    int32_t* hdr = (int32_t*)(ws + 2 * p.rows_bytes + 2 * p.sums_bytes);
    int32_t* perm = hdr + HDR;
    int32_t* key = perm + nq;
    const int pack = VOCR_EXPERIMENT_INT("VOCR_KWS_PACK", 1);     // 0: every query of up to 32 labels takes a wave of its own
    if (launch_class_logprob("vocr_ctc_keyword_scores", logits, lens, canon, clp, t, b, v, s) != VOCR_OK) return VOCR_ELAUNCH;
    not_class_rows_kernel<<<vocr_cdiv((long)t * b, ROWS_PER_BLOCK), 256, 0, s>>>(logits, lens, canon, notc, t, b, v);
    VOCR_CHECK_LAUNCH("vocr_ctc_keyword_scores(not_class)");
    blank_sums_kernel<<<b, 64, 0, s>>>(clp, lens, t, b, v, pre, suf);
    VOCR_CHECK_LAUNCH("vocr_ctc_keyword_scores(blank_sums)");
    keyword_plan_kernel<<<1, 256, 0, s>>>(canon, queries, query_lens, query_flags, v, nq, query_stride, max_query_len, pack, hdr, perm, key);
    VOCR_CHECK_LAUNCH("vocr_ctc_keyword_scores(plan)");
    keyword_search_kernel<<<vocr_cdiv((long)b * nq, 4), 256, 0, s>>>(clp, notc, pre, suf, lens, canon, queries, query_lens, query_flags, t, b,
                                                                    v, nq, query_stride, hdr, perm, out_log_count, out_best, out_span);
    VOCR_CHECK_LAUNCH("vocr_ctc_keyword_scores(search)");
    return VOCR_OK;
}
