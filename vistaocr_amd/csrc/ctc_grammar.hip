// CTC grammar search: for every (line, automaton) the exact probability that the line's collapsed labelling is accepted by a finite
// automaton over the symbol classes, ln P = ln of the sum over all V^len frame paths whose labelling the automaton accepts, and the
// best single (frame path, automaton path) with its labelling.  No beam, no pruning: one sweep over the product of the CTC topology
// with the automaton, frames x (states + arcs) cells.  Conventions are vocr_ctc_align's: blank = 0, classes from canon[V].
//
// An automaton has states 0 .. S-1 (0 the start), accept[s], and arcs a = (src, cls, dst) with non-blank labels, sorted by
// (dst, class, src): the incoming arcs of a state are contiguous and grouped by class.  W[s]: in s, the last frame was blank (or
// nothing was emitted yet); A[a]: the last frame emitted cls_a on arc a.
//   t = 0 :  W[0] = lp_0(blank), A[a] = lp_0(cls_a) if src_a = 0; everything else -inf
//   t > 0 :  W'[s] = lp_t(blank) + lse(W[s], A[a'] for every a' into s)
//            A'[a] = lp_t(cls_a) + lse(A[a], W[src_a], A[a'] for every a' into src_a whose class is not cls_a's)
//   ln P  =  lse(W[s] for accepting s, A[a] for accepting dst_a) after the last frame
// and the same with max for the best path, one back pointer per cell and frame in the workspace.
// TIE RULE (a candidate replaces the choice only when STRICTLY greater): W: stay, then the incoming arcs in arc order; A: stay, then
// W[src], then the incoming arcs in arc order; at the end the accepting W cells in state order, then the arc cells in arc order.
//
//   kernel 1  class log-probabilities : class_logprob_rows_kernel of the alignment.
//   kernel 2  plan                    : one workgroup per automaton validates it and writes, per state, the range of its incoming arcs
//                                       and, per arc, its source, its class and where in the source's incoming arcs the group of its
//                                       own class begins and ends (binary searches over the sorted arcs); and the list of the states
//                                       with 64 or more incoming arcs, in state order.
//   kernel 3  sweep <sum>, <max>      : one workgroup per (line, automaton), sequential over frames, two rows ping-ponging in LDS; the
//                                       automaton's plan is copied into LDS too where it fits beside them (every frame reads all of it).
//             phase 1: per state the exclusive prefix and the inclusive suffix lse (max pass: arg max) over its incoming arcs, so that
//             "all incoming arcs but the group of class c" is lse(prefix at the group's begin, suffix at its end): never a
//             subtraction, O(E) per frame.  A state with fewer than 64 incoming arcs is scanned by one lane, a state with more by a
//             wave (the plan's list, dealt out to the waves in turn), 64 arcs at a time, with (max, sum) pairs through shuffles.
//             phase 2: every W and A cell from the old row and the scans.
// Every float is computed by a fixed lane in a fixed order (no atomics): results are bit-identical from run to run, and the sum pass is
// the same launch with or without best paths.
#include "ctc_align_common.h"

namespace {

constexpr int GN_MAX = 8192;                 // states + arcs of one automaton: two rows and two scans of that many words in LDS
constexpr int WAVE_DEG = 64;                 // incoming arcs from which on a state is scanned by a wave, not by a lane
constexpr int NT_SMALL = 256, NT_BIG = 1024; // threads of a sweep workgroup; NT_BIG when the call's largest automaton exceeds N_SMALL cells
constexpr int N_SMALL = 2048;
constexpr size_t BP_MAX_BYTES = (size_t)1 << 31;
constexpr size_t LDS_DYN_MAX = 160 * 1024 - 13 * 1024;     // what a sweep workgroup may ask for beside its static 12.1 KiB

// words of one automaton's list of wave-scanned states: their number, then the states (each has at least WAVE_DEG arcs of its own)
__host__ __device__ constexpr int big_stride(int max_arcs) { return max_arcs / WAVE_DEG + 2; }

// lower bound over one automaton's arcs: the first i in [lo, hi) with key(i) >= want
template <class Key>
__device__ __forceinline__ int lower_bound(int lo, int hi, int want, Key key) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key(mid) < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// What the weights add to a kernel's arguments; empty without them (the pattern of ctc_beam.hip's Dfa<GRAMMAR>).
template <bool WT>
struct GWeights {};
template <>
struct GWeights<true> {
    const float* __restrict__ arc;              // one natural-log weight per arc, in the order of the arcs the kernel is given
    const float* __restrict__ fin;              // one per state (the caller's state order), read for accepting states only
    const int32_t* __restrict__ accept;
};

__device__ __forceinline__ bool g_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// bytes of one automaton's plan as g_stage lays it out in LDS (the weights, where they are staged too, follow it)
__host__ __device__ constexpr size_t staged_plan_bytes(int max_states, int max_arcs) {
    return (((size_t)max_arcs * sizeof(int4) + (size_t)max_states * sizeof(int2) + (size_t)big_stride(max_arcs) * sizeof(int32_t)) + 15) &
           ~(size_t)15;
}

// grid.x = G, 256 threads.  flags[k] = 1 for an automaton that breaks a rule (nothing else is written for it).  st[k][s] = {first,
// end} of the incoming arcs of s; meta[k][a] = {src, class column, xa, xb}: the other classes' incoming arcs of src are those before
// xa (read: the exclusive prefix at xa; -1: none) and from xb on (the inclusive suffix at xb; -1: none).  arc_stride = 0: automaton k's
// arcs lie at g_arc_off[k] of the arc arrays (the caller's tables); > 0: at k * arc_stride (the mirrored tables in the workspace).
template <bool WT>
__global__ __launch_bounds__(256) void grammar_plan_kernel(const int32_t* __restrict__ canon, const int32_t* __restrict__ g_state_off,
                                                           const int32_t* __restrict__ g_arc_off, const int32_t* __restrict__ arc_src,
                                                           const int32_t* __restrict__ arc_cls, const int32_t* __restrict__ arc_dst, int V,
                                                           int max_states, int max_arcs, int arc_stride,
                                                           int32_t* __restrict__ flags, int2* __restrict__ st, int4* __restrict__ meta,
                                                           int32_t* __restrict__ big_all, GWeights<WT> GW) {
    __shared__ int s_wcnt[4];
    __shared__ int s_base;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int s0 = g_state_off[k], a0 = g_arc_off[k];
    const long S_ = (long)g_state_off[k + 1] - s0, E_ = (long)g_arc_off[k + 1] - a0;
    if (s0 < 0 || a0 < 0 || S_ < 1 || S_ > max_states || E_ < 0 || E_ > max_arcs) {
        if (tid == 0) flags[k] = 1;
        return;
    }
    const int S = (int)S_, E = (int)E_;
    const long base = arc_stride ? (long)k * arc_stride : (long)a0;
    const int32_t* src = arc_src + base;
    const int32_t* cls = arc_cls + base;
    const int32_t* dst = arc_dst + base;
    auto cls_of = [&](int i) { return class_of(canon, min(max(cls[i], 0), V - 1)); };
    int bad = 0;
    for (int i = tid; i < E; i += 256) {
        const int c = cls_of(i);
        bad |= src[i] < 0 || src[i] >= S || dst[i] < 0 || dst[i] >= S || cls[i] <= 0 || cls[i] >= V || c == 0;
        if (i > 0) {
            const int cp = cls_of(i - 1);
            bad |= dst[i - 1] > dst[i] || (dst[i - 1] == dst[i] && (cp > c || (cp == c && src[i - 1] > src[i])));
        }
        if constexpr (WT) bad |= !g_finite(GW.arc[base + i]);
    }
    if constexpr (WT) {                                            // a weight that is NaN or infinite breaks a rule like a mis-sorted arc
        for (int i = tid; i < S; i += 256) bad |= GW.accept[s0 + i] != 0 && !g_finite(GW.fin[s0 + i]);
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) flags[k] = 1;
        return;
    }
    if (tid == 0) {
        flags[k] = 0;
        s_base = 0;
    }
    auto dst_key = [&](int i) { return dst[i]; };
    // the states' ranges, and the list of the states a wave scans, in state order: big[0] their number, big[1 ..] the states
    int32_t* big = big_all + (long)k * big_stride(max_arcs);
    const int lane = tid & 63, w = tid >> 6;
    for (int first = 0; first < S; first += 256) {
        const int s = first + tid;
        int lo = 0, hi = 0;
        if (s < S) {
            lo = lower_bound(0, E, s, dst_key);
            hi = lower_bound(0, E, s + 1, dst_key);
            st[(long)k * max_states + s] = make_int2(lo, hi);
        }
        const bool is_big = hi - lo >= WAVE_DEG;
        const unsigned long long mask = __ballot(is_big);
        if (lane == 0) s_wcnt[w] = __popcll(mask);
        __syncthreads();
        int base = s_base;
        for (int j = 0; j < w; ++j) base += s_wcnt[j];
        if (is_big) big[1 + base + __popcll(mask & ((1ull << lane) - 1ull))] = s;
        __syncthreads();
        if (tid == 0) s_base += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();
    }
    if (tid == 0) big[0] = s_base;
    for (int i = tid; i < E; i += 256) {
        const int s = src[i], c = cls_of(i);
        const int lo = lower_bound(0, E, s, dst_key), hi = lower_bound(0, E, s + 1, dst_key);
        const int g0 = lower_bound(lo, hi, c, cls_of), g1 = lower_bound(lo, hi, c + 1, cls_of);
        int xa = g0 > lo ? g0 : -1, xb = g1 < hi ? g1 : -1;
        if (g0 == g1) { xa = -1; xb = lo < hi ? lo : -1; }        // no arc of that class comes in: the whole range, as one suffix
        meta[(long)k * max_arcs + i] = make_int4(s, c, xa, xb);
    }
}

// one partial result of a scan: the sum pass keeps a logsumexp as (max m, sum s of exp(x - m)), the max pass (value m, arc i)
struct GAcc {
    float m, s;
    int i;
};

__device__ __forceinline__ GAcc g_none() { return {NEG_INF, 0.f, -1}; }
__device__ __forceinline__ GAcc g_elem(float v, int i) { return {v, v == NEG_INF ? 0.f : 1.f, i}; }

// l covers lower arc (cell) indices than r.  max pass: the earlier wins a tie
template <bool BEST>
__device__ __forceinline__ GAcc g_join(const GAcc& l, const GAcc& r) {
    if (BEST) return r.m > l.m ? r : l;
    if (r.m == NEG_INF) return l;
    if (l.m == NEG_INF) return r;
    const float e = expf(-fabsf(l.m - r.m));
    GAcc o;
    o.m = fmaxf(l.m, r.m);
    o.s = l.m >= r.m ? l.s + r.s * e : l.s * e + r.s;
    o.i = -1;
    return o;
}

template <bool BEST>
__device__ __forceinline__ GAcc g_shfl_up(const GAcc& a, int o) {
    GAcc r;
    r.m = __shfl_up(a.m, o, 64);
    r.s = BEST ? 0.f : __shfl_up(a.s, o, 64);
    r.i = BEST ? __shfl_up(a.i, o, 64) : -1;
    return r;
}
template <bool BEST>
__device__ __forceinline__ GAcc g_shfl_down(const GAcc& a, int o) {
    GAcc r;
    r.m = __shfl_down(a.m, o, 64);
    r.s = BEST ? 0.f : __shfl_down(a.s, o, 64);
    r.i = BEST ? __shfl_down(a.i, o, 64) : -1;
    return r;
}
template <bool BEST>
__device__ __forceinline__ GAcc g_shfl(const GAcc& a, int lane) {
    GAcc r;
    r.m = __shfl(a.m, lane, 64);
    r.s = BEST ? 0.f : __shfl(a.s, lane, 64);
    r.i = BEST ? __shfl(a.i, lane, 64) : -1;
    return r;
}

// (a single term: ln 1 = 0, the same bits without the logarithm - every state of a trie)
__device__ __forceinline__ float g_value(const GAcc& a) { return (a.m == NEG_INF || a.s == 1.f) ? a.m : a.m + logf(a.s); }

// a scan entry: the sum pass stores the logsumexp, the max pass the arc of the maximum (its value is read from the row again)
template <bool BEST>
__device__ __forceinline__ void g_store(float* __restrict__ p, int i, const GAcc& a) {
    if (BEST) reinterpret_cast<int*>(p)[i] = a.i;
    else p[i] = g_value(a);
}

// ... read back: the value, and in the max pass the arc it came from (-1: none)
template <bool BEST, bool WT>
__device__ __forceinline__ float g_read(const float* __restrict__ p, int i, const float* __restrict__ A, const float* __restrict__ aw,
                                        int& arc) {
    arc = -1;
    if (i < 0) return NEG_INF;
    if (!BEST) return p[i];
    arc = reinterpret_cast<const int*>(p)[i];
    if (arc < 0) return NEG_INF;
    return WT ? A[arc] + aw[arc] : A[arc];
}

// what arc cell i hands on when it is LEFT: the weighted sweeps pay an arc's weight there (a stay pays nothing)
template <bool WT>
__device__ __forceinline__ float g_out(const float* __restrict__ A, const float* __restrict__ aw, int i) {
    return WT ? A[i] + aw[i] : A[i];
}

// the scans of one state's incoming arcs [lo, hi) by one lane
template <bool BEST, bool WT>
__device__ __forceinline__ void lane_scan(const float* __restrict__ A, const float* __restrict__ aw, float* __restrict__ pre,
                                          float* __restrict__ suf, int lo, int hi) {
    GAcc acc = g_none();
    for (int i = lo; i < hi; ++i) {
        g_store<BEST>(pre, i, acc);
        acc = g_join<BEST>(acc, g_elem(g_out<WT>(A, aw, i), i));
    }
    acc = g_none();
    for (int i = hi - 1; i >= lo; --i) {
        acc = g_join<BEST>(g_elem(g_out<WT>(A, aw, i), i), acc);
        g_store<BEST>(suf, i, acc);
    }
}

// ... and by a whole wave (lo, hi wave-uniform): 64 arcs at a time, Hillis-Steele over the lanes, the earlier chunks carried along
template <bool BEST, bool WT>
__device__ __forceinline__ void wave_scan(const float* __restrict__ A, const float* __restrict__ aw, float* __restrict__ pre,
                                          float* __restrict__ suf, int lo, int hi, int lane) {
    GAcc carry = g_none();
    for (int c0 = lo; c0 < hi; c0 += 64) {
        const int i = c0 + lane;
        GAcc x = i < hi ? g_elem(g_out<WT>(A, aw, i), i) : g_none();
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const GAcc u = g_shfl_up<BEST>(x, o);
            if (lane >= o) x = g_join<BEST>(u, x);
        }
        GAcc ex = g_shfl_up<BEST>(x, 1);
        if (lane == 0) ex = g_none();
        if (i < hi) g_store<BEST>(pre, i, g_join<BEST>(carry, ex));
        carry = g_join<BEST>(carry, g_shfl<BEST>(x, 63));
    }
    carry = g_none();
    for (int c1 = hi; c1 > lo; c1 -= 64) {
        const int i = c1 - 64 + lane;
        GAcc x = i >= lo ? g_elem(g_out<WT>(A, aw, i), i) : g_none();
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const GAcc u = g_shfl_down<BEST>(x, o);
            if (lane + o < 64) x = g_join<BEST>(x, u);
        }
        if (i >= lo) g_store<BEST>(suf, i, g_join<BEST>(x, carry));
        carry = g_join<BEST>(g_shfl<BEST>(x, 0), carry);
    }
}

// What a sweep reads of one automaton: the plan kernel's tables (in global memory, or staged in LDS)
struct GView {
    int S, N;
    const int2* st;
    const int4* meta;
    const int32_t* bigs;
    int nbig;
};

// the plan of automaton k as the plan kernel wrote it
__device__ __forceinline__ GView g_view(int k, int S, int E, const int2* __restrict__ st_all, const int4* __restrict__ meta_all,
                                        const int32_t* __restrict__ big_all, int max_states, int max_arcs) {
    const int32_t* bigs = big_all + (long)k * big_stride(max_arcs);
    return {S, S + E, st_all + (long)k * max_states, meta_all + (long)k * max_arcs, bigs + 1, bigs[0]};
}

// ... copied into LDS at `at` (the caller's threads are past every read of what lay there); ends with a barrier
__device__ __forceinline__ GView g_stage(const GView& g, float* at, int max_states, int max_arcs, int tid, int NT) {
    int4* lm = reinterpret_cast<int4*>(at);
    int2* ls = reinterpret_cast<int2*>(lm + max_arcs);
    int32_t* lb = reinterpret_cast<int32_t*>(ls + max_states);
    for (int i = tid; i < g.N - g.S; i += NT) lm[i] = g.meta[i];
    for (int i = tid; i < g.S; i += NT) ls[i] = g.st[i];
    for (int i = tid; i < g.nbig; i += NT) lb[i] = g.bigs[i];
    __syncthreads();
    return {g.S, g.N, ls, lm, lb, g.nbig};
}

// ... and the automaton's arc weights behind the staged plan (stage & 2: they fit too); else they are read where they lie, one
// coalesced float per arc cell and frame.  No barrier of its own: call it before g_stage, whose barrier covers it.
__device__ __forceinline__ const float* g_stage_weights(const float* __restrict__ aw, int E, int stage, float* stage_at, int max_states,
                                                        int max_arcs, int tid, int NT) {
    if (!(stage & 2)) return aw;
    float* lw = stage_at + staged_plan_bytes(max_states, max_arcs) / sizeof(float);
    for (int i = tid; i < E; i += NT) lw[i] = aw[i];
    return lw;
}

// The first frame's row from its class log-probabilities lpr (in LDS): the W cell of every start state and the arc cells that leave
// one.  start = NULL: state 0 alone (the forward sweep); else start[s] != 0 (the mirrored sweep: every accepting state).
// WT: a start state s of the mirrored sweep carries fw[s], the original's final weight; state 0 of the forward sweep carries none.
template <bool WT>
__device__ __forceinline__ void g_first_row(const GView& g, float* __restrict__ row, const float* __restrict__ lpr,
                                            const int32_t* __restrict__ start, const float* __restrict__ fw, int tid, int NT) {
    for (int c = tid; c < g.N; c += NT) {
        float v = NEG_INF;
        if (c < g.S) {
            if (start ? start[c] != 0 : c == 0) v = lpr[0];
            if (WT && start && v != NEG_INF) v += fw[c];
        } else {
            const int4 m = g.meta[c - g.S];
            if (start ? start[m.x] != 0 : m.x == 0) v = lpr[m.y];
            if (WT && start && v != NEG_INF) v += fw[m.x];
        }
        row[c] = v;
    }
    __syncthreads();
}

// One frame of the recursion: row `nxt` from row `cur`, the frame's class log-probabilities read from lp_row (global) into lpr (LDS)
// on the way.  bp_row (max pass): where each cell came from.  Ends with a barrier: nxt, and lpr, are complete.
// WT: aw[a] is paid when arc cell a is LEFT - every scan entry and every max candidate that comes out of an arc cell is A[a] + aw[a],
// nothing else changes - so a row holds the cells WITHOUT their own arc's weight (the end and the occupancy add it).  In exact
// arithmetic that is the header's "paid on entry" with every arc cell shifted by its own constant: the same ln Z, the same maxima, the
// same candidates in the same order.  The mirrored sweep runs the same code: leaving a mirrored arc is leaving the original one too.
template <bool BEST, bool WT>
__device__ __forceinline__ void g_step(const GView& g, const float* __restrict__ aw, const float* __restrict__ cur, float* __restrict__ nxt, float* __restrict__ pre,
                                       float* __restrict__ suf, float* __restrict__ lpr, const float* __restrict__ lp_row, int V,
                                       int32_t* __restrict__ bp_row, int tid, int NT, int lane, int wave) {
    const int S = g.S, N = g.N;
    const float* A = cur + S;
    const float next_lp = tid < V ? lp_row[tid] : 0.f;             // this frame's row: in LDS after phase 1
    // phase 1: the scans of every state's incoming arcs
    for (int s = tid; s < S; s += NT) {
        const int2 io = g.st[s];
        const int D = io.y - io.x;
        if (D > 0 && D < WAVE_DEG) lane_scan<BEST, WT>(A, aw, pre, suf, io.x, io.y);
    }
    for (int kb = wave; kb < g.nbig; kb += NT >> 6) {              // the states of many incoming arcs, dealt out to the waves
        const int2 io = g.st[g.bigs[kb]];
        wave_scan<BEST, WT>(A, aw, pre, suf, __builtin_amdgcn_readfirstlane(io.x), __builtin_amdgcn_readfirstlane(io.y), lane);
    }
    if (tid < V) lpr[tid] = next_lp;
    __syncthreads();
    // phase 2: every cell
    for (int c = tid; c < N; c += NT) {
        float v;
        int from = c;
        if (c < S) {
            const int2 io = g.st[c];
            int arc;
            const float inc = g_read<BEST, WT>(suf, io.y > io.x ? io.x : -1, A, aw, arc);
            const float w = cur[c];
            if (BEST) {
                v = w;
                if (inc > v) { v = inc; from = S + arc; }
            } else {
                v = lse2(w, inc);
            }
            v += lpr[0];
        } else {
            const int4 m = g.meta[c - S];
            int arc_a, arc_b;
            const float self = cur[c], w = cur[m.x];
            const float pa = g_read<BEST, WT>(pre, m.z, A, aw, arc_a), pb = g_read<BEST, WT>(suf, m.w, A, aw, arc_b);
            if (BEST) {
                v = self;
                if (w > v) { v = w; from = m.x; }
                if (pa > v) { v = pa; from = S + arc_a; }
                if (pb > v) { v = pb; from = S + arc_b; }
            } else {
                const float mx = fmaxf(fmaxf(self, w), fmaxf(pa, pb));
                v = mx == NEG_INF ? NEG_INF : logf(expf(self - mx) + expf(w - mx) + expf(pa - mx) + expf(pb - mx)) + mx;
            }
            v += lpr[m.y];
        }
        nxt[c] = v;
        if (BEST) bp_row[c] = from;
    }
    __syncthreads();
}

// The end: the accepting W cells in state order, then the arc cells with an accepting destination in arc order, joined over the
// workgroup in r_m / r_s / r_i [NT]; the result is their entry 0 (after the last barrier).  len = 0: the start state's flag.
// WT: an accepting W cell adds its state's final weight fw, an arc cell its own arc's weight (it is left here) and fw of its destination.
template <bool BEST, bool WT>
__device__ __forceinline__ void g_finish(const GView& g, const float* __restrict__ aw, const float* __restrict__ fw,
                                         const float* __restrict__ cur, int len, const int32_t* __restrict__ acc_s,
                                         const int32_t* __restrict__ dst, float* r_m, float* r_s, int* r_i, int tid, int NT) {
    GAcc acc = g_none();
    if (len > 0) {
        for (int c = tid; c < g.N; c += NT) {
            const bool fin = c < g.S ? acc_s[c] != 0 : acc_s[dst[c - g.S]] != 0;
            if (!fin) continue;
            float v = cur[c];
            if (WT) v = c < g.S ? v + fw[c] : (v + aw[c - g.S]) + fw[dst[c - g.S]];
            acc = g_join<BEST>(acc, g_elem(v, c));
        }
    } else if (tid == 0 && acc_s[0] != 0) {
        acc = g_elem(WT ? fw[0] : 0.f, 0);
    }
    r_m[tid] = acc.m;
    r_s[tid] = acc.s;
    r_i[tid] = acc.i;
    __syncthreads();
    for (int o = NT >> 1; o > 0; o >>= 1) {
        if (tid < o) {
            const GAcc l = {r_m[tid], r_s[tid], r_i[tid]}, r = {r_m[tid + o], r_s[tid + o], r_i[tid + o]};
            GAcc j;
            if (BEST) j = (r.m > l.m || (r.m == l.m && r.i >= 0 && (l.i < 0 || r.i < l.i))) ? r : l;   // the lower cell wins a tie
            else j = g_join<false>(l, r);
            r_m[tid] = j.m;
            r_s[tid] = j.s;
            r_i[tid] = j.i;
        }
        __syncthreads();
    }
}

// grid.x = B * G, NT_SMALL or NT_BIG threads, dynamic LDS: two rows of maxN cells (states, then arcs), the two scans (maxN words
// each, only E used) and two staged rows of class log-probabilities.  out: out_logp (sum pass) or out_best (max pass).
template <bool BEST, bool WT>
__global__ __launch_bounds__(NT_BIG) void ctc_grammar_kernel(const float* __restrict__ clp, const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ g_state_off, const int32_t* __restrict__ g_arc_off,
                                                             const int32_t* __restrict__ arc_dst, const int32_t* __restrict__ accept,
                                                             const int32_t* __restrict__ flags, const int2* __restrict__ st_all,
                                                             const int4* __restrict__ meta_all, const int32_t* __restrict__ big_all,
                                                             int stage, int T, int B, int V, int G, int max_states, int max_arcs,
                                                             float* __restrict__ out, int32_t* __restrict__ bp_all,
                                                             int32_t* __restrict__ out_labels, int32_t* __restrict__ out_lens,
                                                             int label_stride, GWeights<WT> GW) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float r_m[NT_BIG];
    __shared__ float r_s[NT_BIG];
    __shared__ int r_i[NT_BIG];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int blk = blockIdx.x, b = blk / G, k = blk - b * G;
    const int maxN = max_states + max_arcs;
    int32_t* lab = BEST ? out_labels + (long)blk * label_stride : nullptr;
    if (flags[k]) {                                                // an invalid automaton poisons its own column
        if (tid == 0) {
            out[blk] = NEG_INF;
            if (BEST) out_lens[blk] = -1;
        }
        if (BEST)
            for (int p = tid; p < label_stride; p += NT) lab[p] = 0;
        return;
    }
    const int S = g_state_off[k + 1] - g_state_off[k], E = g_arc_off[k + 1] - g_arc_off[k], N = S + E;
    const int32_t* acc_s = accept + g_state_off[k];
    const int32_t* dst = arc_dst + g_arc_off[k];
    const int len = min(max(lens[b], 0), T);
    GView gv = g_view(k, S, E, st_all, meta_all, big_all, max_states, max_arcs);
    const float* aw = nullptr;                                     // WT: the automaton's arc weights, its states' final weights
    const float* fw = nullptr;
    if constexpr (WT) {
        aw = g_stage_weights(GW.arc + g_arc_off[k], E, stage, sm + 4 * maxN + 2 * VMAX, max_states, max_arcs, tid, NT);
        fw = GW.fin + g_state_off[k];
    }
    if (stage) gv = g_stage(gv, sm + 4 * maxN + 2 * VMAX, max_states, max_arcs, tid, NT);   // every frame reads all of the plan
    const int4* meta = gv.meta;
    float* row0 = sm;
    float* row1 = sm + maxN;
    float* pre = sm + 2 * maxN;
    float* suf = sm + 3 * maxN;
    float* lprow = sm + 4 * maxN;                                  // [2][VMAX]
    int32_t* bp = BEST ? bp_all + (long)blk * T * maxN : nullptr;  // [len][N]: the cell of frame t-1 that cell c of frame t came from
    const long tstride = (long)B * V;
    const float* lpb = clp + (long)b * V;

    if (len > 0) {
        if (tid < V) lprow[tid] = lpb[tid];
        __syncthreads();
        g_first_row<WT>(gv, row0, lprow, nullptr, fw, tid, NT);
    }
    float* cur = row0;
    float* nxt = row1;
    for (int t = 1; t < len; ++t) {
        g_step<BEST, WT>(gv, aw, cur, nxt, pre, suf, lprow + (t & 1) * VMAX, lpb + t * tstride, V, BEST ? bp + (long)t * N : nullptr, tid,
                         NT, lane, wave);
        float* sw = cur;
        cur = nxt;
        nxt = sw;
    }
    g_finish<BEST, WT>(gv, aw, fw, cur, len, acc_s, dst, r_m, r_s, r_i, tid, NT);
    if (!BEST) {
        if (tid == 0) out[blk] = g_value({r_m[0], r_s[0], -1});
        return;
    }
    // the best path, backwards: a label wherever an arc cell is entered from another cell
    const float best = r_m[0];
    __shared__ int s_len;
    if (tid == 0) {
        out[blk] = best;
        int L = -1;
        if (best != NEG_INF) {
            L = 0;
            int c = r_i[0];
            for (int t = len - 1; t >= 0; --t) {
                const int from = t > 0 ? bp[(long)t * N + c] : -1;
                if (c >= S && from != c) lab[L++] = meta[c - S].y;
                c = from;
            }
        }
        out_lens[blk] = L;
        s_len = max(L, 0);
    }
    __syncthreads();
    const int L = s_len;
    for (int p = tid; p < L / 2; p += NT) {                        // the walk wrote the labels last first
        const int u = lab[p];
        lab[p] = lab[L - 1 - p];
        lab[L - 1 - p] = u;
    }
    for (int p = L + tid; p < label_stride; p += NT) lab[p] = 0;
}

struct Plan {
    size_t flags_bytes, st_bytes, meta_bytes, big_bytes, bp_bytes;
    int threads;
    size_t lds;
    int stage;             // 1: the automaton's plan is copied into LDS (it fits beside the rows); | 2: its arc weights too
    bool ok;
    size_t plan_bytes() const { return flags_bytes + st_bytes + meta_bytes + big_bytes; }
};

Plan plan_for(int t, int b, int v, int g, int max_states, int max_arcs, int want_best, bool weighted = false) {
    Plan p = {0, 0, 0, 0, 0, 0, 0, 0, false};
    if (t <= 0 || b <= 0 || v <= 1 || v > VMAX || g < 1 || max_states < 1 || max_arcs < 0) return p;
    if ((long)max_states + max_arcs > GN_MAX || (long)t * b * g >= (1L << 31)) return p;
    const size_t n = (size_t)max_states + max_arcs;
    p.flags_bytes = align16((size_t)g * sizeof(int32_t));
    p.st_bytes = align16((size_t)g * max_states * sizeof(int2));
    p.meta_bytes = align16((size_t)g * max_arcs * sizeof(int4));
    p.big_bytes = align16((size_t)g * big_stride(max_arcs) * sizeof(int32_t));
    if (want_best) {
        p.bp_bytes = (size_t)t * b * g * n * sizeof(int32_t);
        if (p.bp_bytes > BP_MAX_BYTES) return p;
        p.bp_bytes = align16(p.bp_bytes);
    }
    p.threads = n > N_SMALL ? NT_BIG : NT_SMALL;
    p.lds = (4 * n + 2 * VMAX) * sizeof(float);
    const size_t staged = staged_plan_bytes(max_states, max_arcs);
    if (p.lds + staged <= LDS_DYN_MAX) {
        p.stage = 1;
        p.lds += staged;
        const size_t staged_w = align16((size_t)max_arcs * sizeof(float));
        if (weighted && max_arcs > 0 && p.lds + staged_w <= LDS_DYN_MAX) {
            p.stage = 3;
            p.lds += staged_w;
        }
    }
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t vocr_ctc_grammar_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_best) {
    const Plan p = plan_for(t, b, v, g, max_states, max_arcs, want_best);
    if (!p.ok) return 0;
    return clp_bytes(t, b, v) + p.plan_bytes() + p.bp_bytes;
}

namespace {

// both weight tables or neither, under the entry's name
int check_weight_tables(const char* who, const float* arc_logw, const float* final_logw) {
    VOCR_CHECK_ARG(!arc_logw == !final_logw, "%s: arc_logw and final_logw go together (arc_logw %s, final_logw %s)", who,
                   arc_logw ? "given" : "NULL", final_logw ? "given" : "NULL");
    return VOCR_OK;
}

// what vocr_ctc_grammar_scores and vocr_ctc_grammar_scores_weighted do: WT = false is the code the unweighted entry always ran
template <bool WT>
int grammar_scores(const char* who, const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                   const int32_t* g_state_off, const int32_t* g_arc_off, int g, const int32_t* arc_src, const int32_t* arc_cls,
                   const int32_t* arc_dst, const int32_t* accept, GWeights<WT> GW, int max_states, int max_arcs, float* out_logp,
                   float* out_best, int32_t* out_labels, int32_t* out_lens, int label_stride, void* workspace, size_t workspace_bytes,
                   void* stream) {
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 1 && v <= VMAX, "%s: need t > 0, b > 0, 2 <= v <= %d (t=%d b=%d v=%d)", who, VMAX, t, b, v);
    VOCR_CHECK_ARG(g >= 1, "%s: need g >= 1 (g=%d)", who, g);
    VOCR_CHECK_ARG(max_states >= 1 && max_arcs >= 0 && (long)max_states + max_arcs <= GN_MAX,
                   "%s: need max_states >= 1, max_arcs >= 0 and max_states + max_arcs <= %d (max_states=%d max_arcs=%d)", who, GN_MAX,
                   max_states, max_arcs);
    const bool any_best = out_best || out_labels || out_lens, all_best = out_best && out_labels && out_lens;
    VOCR_CHECK_ARG(any_best == all_best, "%s: out_best, out_labels and out_lens must be all NULL or all given", who);
    VOCR_CHECK_ARG(!all_best || label_stride >= t, "%s: need label_stride >= t (label_stride=%d t=%d)", who, label_stride, t);
    const Plan p = plan_for(t, b, v, g, max_states, max_arcs, all_best ? 1 : 0, WT);
    VOCR_CHECK_ARG(p.ok, "%s: unsupported shape (t=%d b=%d v=%d g=%d max_states=%d max_arcs=%d): t*b*g must stay below 2^31 and the back "
                   "pointers, t*b*g*(max_states+max_arcs)*4 bytes, within 2 GiB", who, t, b, v, g, max_states, max_arcs);
    VOCR_CHECK_ARG(logits && lens && g_state_off && g_arc_off && accept && out_logp && workspace && (max_arcs == 0 || (arc_src && arc_cls && arc_dst)),
                   "%s: null pointer", who);
    const size_t need = clp_bytes(t, b, v) + p.plan_bytes() + p.bp_bytes;
    VOCR_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    VOCR_CHECK_ARG((((uintptr_t)workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_grammar_kernel<false, WT>, (const void*)ctc_grammar_kernel<true, WT>};
    if (vocr_allow_dynamic_lds(big, 2, (int)LDS_DYN_MAX, &lds_set, who) != VOCR_OK) return VOCR_ELAUNCH;
    char* ws = (char*)workspace;
    float* clp = (float*)ws;
    int32_t* flags = (int32_t*)(ws + clp_bytes(t, b, v));
    int2* st = (int2*)((char*)flags + p.flags_bytes);
    int4* meta = (int4*)((char*)st + p.st_bytes);
    int32_t* bigs = (int32_t*)((char*)meta + p.meta_bytes);
    int32_t* bp = (int32_t*)((char*)bigs + p.big_bytes);
    if (launch_class_logprob(who, logits, lens, canon, clp, t, b, v, s) != VOCR_OK) return VOCR_ELAUNCH;
    grammar_plan_kernel<WT><<<g, 256, 0, s>>>(canon, g_state_off, g_arc_off, arc_src, arc_cls, arc_dst, v, max_states, max_arcs, 0, flags,
                                              st, meta, bigs, GW);
    VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_scores_weighted(plan)" : "vocr_ctc_grammar_scores(plan)");
    ctc_grammar_kernel<false, WT><<<b * g, p.threads, p.lds, s>>>(clp, lens, g_state_off, g_arc_off, arc_dst, accept, flags, st, meta, bigs,
                                                                 p.stage, t, b, v, g, max_states, max_arcs, out_logp, nullptr, nullptr,
                                                                 nullptr, 0, GW);
    VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_scores_weighted(sum)" : "vocr_ctc_grammar_scores(sum)");
    if (all_best) {
        ctc_grammar_kernel<true, WT><<<b * g, p.threads, p.lds, s>>>(clp, lens, g_state_off, g_arc_off, arc_dst, accept, flags, st, meta,
                                                                    bigs, p.stage, t, b, v, g, max_states, max_arcs, out_best, bp,
                                                                    out_labels, out_lens, label_stride, GW);
        VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_scores_weighted(max)" : "vocr_ctc_grammar_scores(max)");
    }
    return VOCR_OK;
}

}  // namespace

extern "C" int vocr_ctc_grammar_scores(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                       const int32_t* g_state_off, const int32_t* g_arc_off, int g, const int32_t* arc_src,
                                       const int32_t* arc_cls, const int32_t* arc_dst, const int32_t* accept, int max_states, int max_arcs,
                                       float* out_logp, float* out_best, int32_t* out_labels, int32_t* out_lens, int label_stride,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    return grammar_scores<false>("vocr_ctc_grammar_scores", logits, lens, t, b, v, canon, g_state_off, g_arc_off, g, arc_src, arc_cls,
                                 arc_dst, accept, {}, max_states, max_arcs, out_logp, out_best, out_labels, out_lens, label_stride,
                                 workspace, workspace_bytes, stream);
}

// The same with weights on the arcs and on the accepting states (the header above; "paid on leaving": g_step).  The workspace is the
// unweighted entry's: the weights are read where the caller keeps them, or staged in LDS.
extern "C" size_t vocr_ctc_grammar_weighted_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_best) {
    return vocr_ctc_grammar_workspace_bytes(t, b, v, g, max_states, max_arcs, want_best);
}

extern "C" int vocr_ctc_grammar_scores_weighted(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                                const int32_t* g_state_off, const int32_t* g_arc_off, int g, const int32_t* arc_src,
                                                const int32_t* arc_cls, const int32_t* arc_dst, const int32_t* accept,
                                                const float* arc_logw, const float* final_logw, int max_states, int max_arcs,
                                                float* out_logp, float* out_best, int32_t* out_labels, int32_t* out_lens,
                                                int label_stride, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "vocr_ctc_grammar_scores_weighted";
    if (const int rc = check_weight_tables(who, arc_logw, final_logw)) return rc;
    if (!arc_logw)
        return grammar_scores<false>(who, logits, lens, t, b, v, canon, g_state_off, g_arc_off, g, arc_src, arc_cls, arc_dst, accept, {},
                                     max_states, max_arcs, out_logp, out_best, out_labels, out_lens, label_stride, workspace,
                                     workspace_bytes, stream);
    return grammar_scores<true>(who, logits, lens, t, b, v, canon, g_state_off, g_arc_off, g, arc_src, arc_cls, arc_dst, accept,
                                {arc_logw, final_logw, accept}, max_states, max_arcs, out_logp, out_best, out_labels, out_lens,
                                label_stride, workspace, workspace_bytes, stream);
}

// ---- vocr_ctc_grammar_grad: ln P of line b under automaton which[b], and its gradient with respect to the logits ----
// The product graph is symmetric under reversal: bhat_t(c), the log-sum over the accepted continuations that start in cell c at frame t
// (frame t's emission included), is the SAME recursion (g_first_row, g_step) over the mirrored automaton - arcs (dst, cls, src), sorted
// by (src, class, dst), every accepting state a start - on the frames read backwards.
//   kernel M  mirror   : one workgroup per automaton sorts its arcs by (src, class, dst, arc) - a bitonic sort of 64-bit keys in the
//                        workspace - and writes the mirrored tables and perm[r] = the arc behind mirrored arc r; then sorts the mirrored
//                        arcs by (class, r): cpos[r] = r's place in that order, cbeg[k] = where class k begins in it.
//                        grammar_plan_kernel runs on the result.
//   kernel G  sweep    : one workgroup per LINE.  Forward: ctc_grammar_kernel<false>'s frame loop and end, every row also stored
//                        [len][maxN] in the workspace.  Backward: per frame the bhat row, then z(c) = exp(alpha + bhat - lp - ln P)
//                        into LDS in class-sorted order (the words of the prefix scan, free between two steps), occ(k) = the sum
//                        over class k's slots by one wave per class (lanes stride, then a butterfly: a fixed order), left in the
//                        line's row of dlogits.  No beta lattice is stored, and no load from global memory is on the frame loop's
//                        critical path: the cells' tables are in registers, the forward row is loaded ahead of the step.
//   kernel R  rows     : one wave per row turns the occupancies into dlogits in vocr_ctc_nbest_grad's form.
namespace {

constexpr int IDX_BITS = 13;                 // GN_MAX = 2^13: a state or an arc index
constexpr int IDX_MASK = (1 << IDX_BITS) - 1;
constexpr size_t LATTICE_MAX_BYTES = (size_t)1 << 31;
constexpr int CPT = GN_MAX / NT_BIG;         // cells a thread of the gradient sweep owns at most: N_SMALL / NT_SMALL is the same 8
static_assert(CPT * NT_SMALL >= N_SMALL && CPT * NT_BIG >= GN_MAX, "a thread's cells");

// ascending bitonic sort of p2 (a power of two) keys in global memory by one workgroup; ends with a barrier
__device__ __forceinline__ void g_sort(unsigned long long* keys, int p2, int tid, int NT) {
    for (int k2 = 2; k2 <= p2; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < p2; i += NT) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k2) == 0)) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
            }
            __syncthreads();
        }
}

// grid.x = G.  Nothing is written for an automaton whose offsets break a rule (the plan kernel flags it from the same test); one
// that breaks another rule gets tables that stay within bounds and are never swept.  WT: m_logw[r] = the weight of the arc behind
// mirrored arc r - the weights are permuted with the arcs.
template <bool WT>
__global__ __launch_bounds__(NT_BIG) void grammar_mirror_kernel(const int32_t* __restrict__ canon, const int32_t* __restrict__ g_state_off,
                                                                const int32_t* __restrict__ g_arc_off, const int32_t* __restrict__ arc_src,
                                                                const int32_t* __restrict__ arc_cls, const int32_t* __restrict__ arc_dst,
                                                                int V, int max_states, int max_arcs, int p2max,
                                                                unsigned long long* keys_all, int32_t* m_src, int32_t* m_cls,
                                                                int32_t* m_dst, int32_t* perm_all, int32_t* cpos_all, int32_t* cbeg_all,
                                                                GWeights<WT> GW, float* m_logw) {
    const int k = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int s0 = g_state_off[k], a0 = g_arc_off[k];
    const long S_ = (long)g_state_off[k + 1] - s0, E_ = (long)g_arc_off[k + 1] - a0;
    if (s0 < 0 || a0 < 0 || S_ < 1 || S_ > max_states || E_ < 0 || E_ > max_arcs) return;
    const int E = (int)E_;
    const int32_t* src = arc_src + a0;
    const int32_t* cls = arc_cls + a0;
    const int32_t* dst = arc_dst + a0;
    unsigned long long* keys = keys_all + (long)k * p2max;
    int32_t* ms = m_src + (long)k * max_arcs;
    int32_t* mc = m_cls + (long)k * max_arcs;
    int32_t* md = m_dst + (long)k * max_arcs;
    int32_t* perm = perm_all + (long)k * max_arcs;
    int32_t* cpos = cpos_all + (long)k * max_arcs;
    int32_t* cbeg = cbeg_all + (long)k * (VMAX + 1);
    int p2 = 1;
    while (p2 < E) p2 <<= 1;                                       // <= p2max: E <= max_arcs
    for (int i = tid; i < p2; i += NT) {
        unsigned long long key = ~0ull;
        if (i < E) {
            const unsigned long long c = (unsigned long long)class_of(canon, min(max(cls[i], 0), V - 1));
            key = ((unsigned long long)(src[i] & IDX_MASK) << (2 * IDX_BITS + 8)) | (c << (2 * IDX_BITS)) |
                  ((unsigned long long)(dst[i] & IDX_MASK) << IDX_BITS) | (unsigned long long)i;
        }
        keys[i] = key;
    }
    __syncthreads();
    g_sort(keys, p2, tid, NT);
    for (int r = tid; r < E; r += NT) {
        const int i = (int)(keys[r] & IDX_MASK);
        ms[r] = dst[i];
        mc[r] = cls[i];
        md[r] = src[i];
        perm[r] = i;
        if constexpr (WT) m_logw[(long)k * max_arcs + r] = GW.arc[a0 + i];
    }
    __syncthreads();
    for (int r = tid; r < p2; r += NT) {
        unsigned long long key = ~0ull;
        if (r < E) key = ((unsigned long long)class_of(canon, min(max(mc[r], 0), V - 1)) << IDX_BITS) | (unsigned long long)r;
        keys[r] = key;
    }
    __syncthreads();
    g_sort(keys, p2, tid, NT);
    __syncthreads();                                               // (a single key is not sorted: no barrier in there)
    for (int j = tid; j < E; j += NT) cpos[(int)(keys[j] & IDX_MASK)] = j;
    auto cls_key = [&](int j) { return (int)(keys[j] >> IDX_BITS); };
    for (int c = tid; c <= V; c += NT) cbeg[c] = lower_bound(0, E, c, cls_key);
}

// rows [t0, T) of line b as zeros
__device__ __forceinline__ void g_zero_rows(float* __restrict__ dlogits, int b, int t0, int T, int B, int V, int tid, int NT) {
    for (long i = tid; i < (long)(T - t0) * V; i += NT) {
        const long t = t0 + i / V;
        dlogits[(t * B + b) * V + i % V] = 0.f;
    }
}

// grid.x = B, NT_SMALL or NT_BIG threads, ctc_grammar_kernel's dynamic LDS.  dlogits = NULL: scores only (lat and the mirrored
// plan are not touched); else the rows of a line with a score hold occ(t, k) behind it, every other row zeros.
template <bool WT>
__global__ __launch_bounds__(NT_BIG) void ctc_grammar_grad_kernel(
    const float* __restrict__ clp, const int32_t* __restrict__ lens, const int32_t* __restrict__ g_state_off, const int32_t* __restrict__ g_arc_off, const int32_t* __restrict__ arc_dst,
    const int32_t* __restrict__ accept, const int32_t* __restrict__ which,
    const int32_t* __restrict__ flags_f, const int2* __restrict__ st_f, const int4* __restrict__ meta_f, const int32_t* __restrict__ big_f,
    const int32_t* __restrict__ flags_m, const int2* __restrict__ st_m, const int4* __restrict__ meta_m, const int32_t* __restrict__ big_m,
    const int32_t* __restrict__ perm_all, const int32_t* __restrict__ cpos_all, const int32_t* __restrict__ cbeg_all, int stage, int T,
    int B, int V, int G, int max_states, int max_arcs, float* __restrict__ out_logp, float* __restrict__ lat, float* __restrict__ dlogits,
    GWeights<WT> GW, const float* __restrict__ m_logw) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float r_m[NT_BIG];
    __shared__ float r_s[NT_BIG];
    __shared__ int r_i[NT_BIG];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, k = which[b];
    const int maxN = max_states + max_arcs;
    bool bad = k < 0 || k >= G;
    if (!bad) bad = flags_f[k] != 0 || (dlogits && flags_m[k] != 0);
    if (bad) {                                                     // poisons its own line alone
        if (tid == 0) out_logp[b] = NEG_INF;
        if (dlogits) g_zero_rows(dlogits, b, 0, T, B, V, tid, NT);
        return;
    }
    const int S = g_state_off[k + 1] - g_state_off[k], E = g_arc_off[k + 1] - g_arc_off[k], N = S + E;
    const int32_t* acc_s = accept + g_state_off[k];
    const int32_t* dst = arc_dst + g_arc_off[k];
    const int len = min(max(lens[b], 0), T);
    float* stage_at = sm + 4 * maxN + 2 * VMAX;
    GView gv = g_view(k, S, E, st_f, meta_f, big_f, max_states, max_arcs);
    const float* aw = nullptr;                                     // WT: the arc weights of the sweep at hand, the states' final weights
    const float* fw = nullptr;
    if constexpr (WT) {
        aw = g_stage_weights(GW.arc + g_arc_off[k], E, stage, stage_at, max_states, max_arcs, tid, NT);
        fw = GW.fin + g_state_off[k];
    }
    if (stage) gv = g_stage(gv, stage_at, max_states, max_arcs, tid, NT);
    float* row0 = sm;
    float* row1 = sm + maxN;
    float* pre = sm + 2 * maxN;
    float* suf = sm + 3 * maxN;
    float* lprow = sm + 4 * maxN;                                  // [2][VMAX]
    const long tstride = (long)B * V;
    const float* lpb = clp + (long)b * V;
    float* lat_b = dlogits ? lat + (long)b * T * maxN : nullptr;   // [len][maxN]: the forward rows

    // forward: ctc_grammar_kernel<false>, frame for frame
    if (len > 0) {
        if (tid < V) lprow[tid] = lpb[tid];
        __syncthreads();
        g_first_row<WT>(gv, row0, lprow, nullptr, fw, tid, NT);
        if (lat_b)
            for (int c = tid; c < N; c += NT) lat_b[c] = row0[c];
    }
    float* cur = row0;
    float* nxt = row1;
    for (int t = 1; t < len; ++t) {
        g_step<false, WT>(gv, aw, cur, nxt, pre, suf, lprow + (t & 1) * VMAX, lpb + t * tstride, V, nullptr, tid, NT, lane, wave);
        float* sw = cur;
        cur = nxt;
        nxt = sw;
        if (lat_b)
            for (int c = tid; c < N; c += NT) lat_b[(long)t * maxN + c] = cur[c];
    }
    g_finish<false, WT>(gv, aw, fw, cur, len, acc_s, dst, r_m, r_s, r_i, tid, NT);
    const float lnP = g_value({r_m[0], r_s[0], -1});
    if (tid == 0) out_logp[b] = lnP;
    if (!dlogits) return;
    if (lnP == NEG_INF || len == 0) {
        g_zero_rows(dlogits, b, 0, T, B, V, tid, NT);
        return;
    }
    __syncthreads();                                               // every thread has read ln P: the reduction's arrays are free
    int* cb = reinterpret_cast<int*>(r_m);                         // [V + 1]: where class k begins among the class-sorted arc cells
    const int32_t* cbeg = cbeg_all + (long)k * (VMAX + 1);
    for (int i = tid; i <= V; i += NT) cb[i] = cbeg[i];

    // backward: the same recursion over the mirrored automaton (the forward's staged plan is dead by now), the occupancy folded in.
    // Nothing in the frame loop waits for global memory: what a thread needs of its cells c = tid + i NT (at most CPT of them:
    // N <= CPT * NT at both thread counts) is in registers before it starts, and the forward row of frame t is loaded ahead of
    // the step that makes frame t's bhat.
    // WT: alpha and bhat of an arc cell both leave its own weight out (it is paid on leaving, in either direction), every other weight
    // of a path through the cell is in exactly one of them - the earlier arcs' in alpha, the later arcs' and the final weight (the
    // mirrored sweep's start weight) in bhat - so the occupancy adds the cell's own weight, once.
    gv = g_view(k, S, E, st_m, meta_m, big_m, max_states, max_arcs);
    if constexpr (WT) aw = g_stage_weights(m_logw + (long)k * max_arcs, E, stage, stage_at, max_states, max_arcs, tid, NT);
    if (stage) gv = g_stage(gv, stage_at, max_states, max_arcs, tid, NT);
    const int32_t* perm = perm_all + (long)k * max_arcs;
    const int32_t* cpos = cpos_all + (long)k * max_arcs;
    int ai[CPT], zi[CPT], ecol[CPT];                               // the cell's word in a forward row, its slot among the class-sorted z, its class
    float wz[WT ? CPT : 1];                                        // WT: the cell's own arc weight (0 for a W cell)
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int c = tid + i * NT;
        ai[i] = -1;
        zi[i] = ecol[i] = 0;
        if constexpr (WT) wz[i] = 0.f;
        if (c < S) {
            ai[i] = zi[i] = c;
        } else if (c < N) {
            ai[i] = S + perm[c - S];
            zi[i] = S + cpos[c - S];
            ecol[i] = gv.meta[c - S].y;
            if constexpr (WT) wz[i] = aw[c - S];
        }
    }
    if (tid < V) lprow[tid] = lpb[(long)(len - 1) * tstride + tid];
    __syncthreads();
    g_first_row<WT>(gv, row0, lprow, acc_s, fw, tid, NT);
    cur = row0;
    nxt = row1;
    for (int j = 0; j < len; ++j) {
        const int t = len - 1 - j;
        const float* lpr = lprow + (j & 1) * VMAX;
        const float* al = lat_b + (long)t * maxN;
        float a[CPT];
#pragma unroll
        for (int i = 0; i < CPT; ++i) a[i] = ai[i] >= 0 ? al[ai[i]] : NEG_INF;
        if (j > 0) {
            g_step<false, WT>(gv, aw, cur, nxt, pre, suf, lprow + (j & 1) * VMAX, lpb + t * tstride, V, nullptr, tid, NT, lane, wave);
            float* sw = cur;
            cur = nxt;
            nxt = sw;
        }
#pragma unroll
        for (int i = 0; i < CPT; ++i) {                            // z(c): the share of the accepted mass that passes through c at t
            if (ai[i] < 0) continue;
            const float bh = cur[tid + i * NT];
            float ab = a[i] + bh;
            if constexpr (WT) ab += wz[i];
            pre[zi[i]] = (a[i] == NEG_INF || bh == NEG_INF) ? 0.f : expf(ab - lpr[ecol[i]] - lnP);
        }
        __syncthreads();
        float* occ_row = dlogits + ((long)t * B + b) * V;          // occ(t, k) waits here for the row kernel
        for (int kc = wave; kc < V; kc += NT >> 6) {               // one wave per class over its slots, a fixed order
            const int q0 = kc == 0 ? 0 : S + cb[kc], q1 = kc == 0 ? S : S + cb[kc + 1];
            float s = 0.f;
            for (int q = q0 + lane; q < q1; q += 64) s += pre[q];
            s = wave_sum(s);
            if (lane == 0) occ_row[kc] = s;
        }
        __syncthreads();                                           // the next step's scans write pre
    }
    g_zero_rows(dlogits, b, len, T, B, V, tid, NT);
}

// grid.x = ceil(T B / 4), 256 threads: one wave per row (t, b) turns the row of class occupancies the sweep left in dlogits into the
// row of the gradient, share * (w occ) - p w, in ctc_grad_rows' arithmetic.  Rows the sweep wrote as zeros are left alone.
__global__ __launch_bounds__(256) void grammar_grad_rows_kernel(const float* __restrict__ logits, const float* __restrict__ clp,
                                                                const int32_t* __restrict__ lens, const int32_t* __restrict__ canon,
                                                                const float* __restrict__ weights, const float* __restrict__ out_logp,
                                                                int T, int B, int V, float* __restrict__ dlogits) {
    __shared__ float s_occ[4][VMAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= (long)T * B) return;
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    if (t >= min(max(lens[b], 0), T) || out_logp[b] == NEG_INF) return;
    float* out = dlogits + row * V;
    float* occ = s_occ[wave];
    for (int v = lane; v < V; v += 64) occ[v] = out[v];
    __builtin_amdgcn_wave_barrier();
    const float* xr = logits + row * V;
    const float* cr = clp + row * V;
    const float w = weights[b];
    const RowLse rl = wave_row_lse(xr, V, lane);                   // the bits of class_logprob_rows_kernel's log-softmax
    for (int v = lane; v < V; v += 64) {
        const float lpv = row_logprob(rl, xr, v);
        const float share = (lpv == NEG_INF) ? 0.f : expf(lpv - cr[v]);          // p_t(v) / P_t(class(v))
        out[v] = share * (w * occ[class_of(canon, v)]) - expf(lpv) * w;
    }
}

struct GradPlan {
    Plan p;
    int p2;                // one automaton's sort keys: max_arcs rounded up to a power of two
    size_t arcs_bytes, keys_bytes, cbeg_bytes, lattice_bytes;
    bool ok;
    size_t mirror_bytes() const { return 5 * arcs_bytes + keys_bytes + cbeg_bytes + p.plan_bytes(); }
};

GradPlan grad_plan_for(int t, int b, int v, int g, int max_states, int max_arcs, int want_grad, bool weighted = false) {
    GradPlan q = {plan_for(t, b, v, g, max_states, max_arcs, 0, weighted), 1, 0, 0, 0, 0, false};
    if (!q.p.ok) return q;
    q.ok = true;
    if (!want_grad) return q;
    while (q.p2 < max_arcs) q.p2 <<= 1;
    q.arcs_bytes = align16((size_t)g * max_arcs * sizeof(int32_t));
    q.keys_bytes = align16((size_t)g * q.p2 * sizeof(unsigned long long));
    q.cbeg_bytes = align16((size_t)g * (VMAX + 1) * sizeof(int32_t));
    q.lattice_bytes = (size_t)t * b * ((size_t)max_states + max_arcs) * sizeof(float);
    if (q.lattice_bytes > LATTICE_MAX_BYTES) q.ok = false;
    q.lattice_bytes = align16(q.lattice_bytes);
    return q;
}

// what both gradient entries need; the weighted entry (weighted_entry) keeps the mirrored weights behind everything else
size_t grad_need(const GradPlan& q, int t, int b, int v, int want_grad, bool weighted_entry) {
    return clp_bytes(t, b, v) + q.p.plan_bytes() + (want_grad ? q.mirror_bytes() + q.lattice_bytes + (weighted_entry ? q.arcs_bytes : 0) : 0);
}

}  // namespace

extern "C" size_t vocr_ctc_grammar_grad_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_grad) {
    const GradPlan q = grad_plan_for(t, b, v, g, max_states, max_arcs, want_grad);
    if (!q.ok) return 0;
    return grad_need(q, t, b, v, want_grad, false);
}

// the weighted entry's: one more float per arc slot, the mirrored weights
extern "C" size_t vocr_ctc_grammar_grad_weighted_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_grad) {
    const GradPlan q = grad_plan_for(t, b, v, g, max_states, max_arcs, want_grad);
    if (!q.ok) return 0;
    return grad_need(q, t, b, v, want_grad, true);
}

namespace {

// what vocr_ctc_grammar_grad and vocr_ctc_grammar_grad_weighted do: WT = false is the code the unweighted entry always ran, in the
// same workspace layout (weighted_entry only asks for the mirrored weights' room behind it)
template <bool WT>
int grammar_grad(const char* who, bool weighted_entry, const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                 const int32_t* g_state_off, const int32_t* g_arc_off, int g, const int32_t* arc_src, const int32_t* arc_cls,
                 const int32_t* arc_dst, const int32_t* accept, GWeights<WT> GW, int max_states, int max_arcs, const int32_t* which,
                 const float* weights, float* out_logp, float* dlogits, void* workspace, size_t workspace_bytes, void* stream) {
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 1 && v <= VMAX, "%s: need t > 0, b > 0, 2 <= v <= %d (t=%d b=%d v=%d)", who, VMAX, t, b, v);
    VOCR_CHECK_ARG(g >= 1, "%s: need g >= 1 (g=%d)", who, g);
    VOCR_CHECK_ARG(max_states >= 1 && max_arcs >= 0 && (long)max_states + max_arcs <= GN_MAX,
                   "%s: need max_states >= 1, max_arcs >= 0 and max_states + max_arcs <= %d (max_states=%d max_arcs=%d)", who, GN_MAX,
                   max_states, max_arcs);
    VOCR_CHECK_ARG(!weights == !dlogits, "%s: weights and dlogits go together (weights %s, dlogits %s)", who, weights ? "given" : "NULL",
                   dlogits ? "given" : "NULL");
    const int want_grad = dlogits ? 1 : 0;
    const GradPlan q = grad_plan_for(t, b, v, g, max_states, max_arcs, want_grad, WT);
    VOCR_CHECK_ARG(q.ok, "%s: unsupported shape (t=%d b=%d v=%d g=%d max_states=%d max_arcs=%d): t*b*g must stay below 2^31 and the stored "
                   "lattice, t*b*(max_states+max_arcs)*4 bytes, within 2 GiB", who, t, b, v, g, max_states, max_arcs);
    VOCR_CHECK_ARG(logits && lens && g_state_off && g_arc_off && accept && which && out_logp && workspace &&
                   (max_arcs == 0 || (arc_src && arc_cls && arc_dst)), "%s: null pointer", who);
    const size_t need = grad_need(q, t, b, v, want_grad, weighted_entry);
    VOCR_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    VOCR_CHECK_ARG((((uintptr_t)workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_grammar_grad_kernel<WT>};
    if (vocr_allow_dynamic_lds(big, 1, (int)LDS_DYN_MAX, &lds_set, who) != VOCR_OK) return VOCR_ELAUNCH;
    const Plan& p = q.p;
    char* at = (char*)workspace;
    auto take = [&](size_t bytes) {
        char* r = at;
        at += bytes;
        return r;
    };
    float* clp = (float*)take(clp_bytes(t, b, v));
    int32_t* flags = (int32_t*)take(p.flags_bytes);
    int2* st = (int2*)take(p.st_bytes);
    int4* meta = (int4*)take(p.meta_bytes);
    int32_t* bigs = (int32_t*)take(p.big_bytes);
    if (launch_class_logprob(who, logits, lens, canon, clp, t, b, v, s) != VOCR_OK) return VOCR_ELAUNCH;
    grammar_plan_kernel<WT><<<g, 256, 0, s>>>(canon, g_state_off, g_arc_off, arc_src, arc_cls, arc_dst, v, max_states, max_arcs, 0, flags,
                                              st, meta, bigs, GW);
    VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_grad_weighted(plan)" : "vocr_ctc_grammar_grad(plan)");
    int32_t *flags_m = nullptr, *bigs_m = nullptr, *perm = nullptr, *cpos = nullptr, *cbeg = nullptr;
    int2* st_m = nullptr;
    int4* meta_m = nullptr;
    float* lat = nullptr;
    float* m_logw = nullptr;
    if (want_grad) {
        flags_m = (int32_t*)take(p.flags_bytes);
        st_m = (int2*)take(p.st_bytes);
        meta_m = (int4*)take(p.meta_bytes);
        bigs_m = (int32_t*)take(p.big_bytes);
        unsigned long long* keys = (unsigned long long*)take(q.keys_bytes);
        int32_t* m_src = (int32_t*)take(q.arcs_bytes);
        int32_t* m_cls = (int32_t*)take(q.arcs_bytes);
        int32_t* m_dst = (int32_t*)take(q.arcs_bytes);
        perm = (int32_t*)take(q.arcs_bytes);
        cpos = (int32_t*)take(q.arcs_bytes);
        cbeg = (int32_t*)take(q.cbeg_bytes);
        lat = (float*)take(q.lattice_bytes);
        if (WT) m_logw = (float*)take(q.arcs_bytes);
        grammar_mirror_kernel<WT><<<g, max_arcs > 1024 ? NT_BIG : NT_SMALL, 0, s>>>(canon, g_state_off, g_arc_off, arc_src, arc_cls, arc_dst,
                                                                                   v, max_states, max_arcs, q.p2, keys, m_src, m_cls, m_dst,
                                                                                   perm, cpos, cbeg, GW, m_logw);
        VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_grad_weighted(mirror)" : "vocr_ctc_grammar_grad(mirror)");
        // (the forward plan has judged the weights: the mirrored plan checks the arcs alone)
        grammar_plan_kernel<false><<<g, 256, 0, s>>>(canon, g_state_off, g_arc_off, m_src, m_cls, m_dst, v, max_states, max_arcs,
                                                     max_arcs > 0 ? max_arcs : 1, flags_m, st_m, meta_m, bigs_m, {});
        VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_grad_weighted(mirrored plan)" : "vocr_ctc_grammar_grad(mirrored plan)");
    }
    ctc_grammar_grad_kernel<WT><<<b, p.threads, p.lds, s>>>(clp, lens, g_state_off, g_arc_off, arc_dst, accept, which, flags, st, meta, bigs,
                                                            flags_m, st_m, meta_m, bigs_m, perm, cpos, cbeg, p.stage, t, b, v, g, max_states,
                                                            max_arcs, out_logp, lat, dlogits, GW, m_logw);
    VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_grad_weighted(sweep)" : "vocr_ctc_grammar_grad(sweep)");
    if (want_grad) {
        grammar_grad_rows_kernel<<<vocr_cdiv((long)t * b, 4), 256, 0, s>>>(logits, clp, lens, canon, weights, out_logp, t, b, v, dlogits);
        VOCR_CHECK_LAUNCH(WT ? "vocr_ctc_grammar_grad_weighted(rows)" : "vocr_ctc_grammar_grad(rows)");
    }
    return VOCR_OK;
}

}  // namespace

extern "C" int vocr_ctc_grammar_grad(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                     const int32_t* g_state_off, const int32_t* g_arc_off, int g, const int32_t* arc_src,
                                     const int32_t* arc_cls, const int32_t* arc_dst, const int32_t* accept, int max_states, int max_arcs,
                                     const int32_t* which, const float* weights, float* out_logp, float* dlogits, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return grammar_grad<false>("vocr_ctc_grammar_grad", false, logits, lens, t, b, v, canon, g_state_off, g_arc_off, g, arc_src, arc_cls,
                               arc_dst, accept, {}, max_states, max_arcs, which, weights, out_logp, dlogits, workspace, workspace_bytes,
                               stream);
}

extern "C" int vocr_ctc_grammar_grad_weighted(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                              const int32_t* g_state_off, const int32_t* g_arc_off, int g, const int32_t* arc_src,
                                              const int32_t* arc_cls, const int32_t* arc_dst, const int32_t* accept, const float* arc_logw,
                                              const float* final_logw, int max_states, int max_arcs, const int32_t* which,
                                              const float* weights, float* out_logp, float* dlogits, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    const char* who = "vocr_ctc_grammar_grad_weighted";
    if (const int rc = check_weight_tables(who, arc_logw, final_logw)) return rc;
    if (!arc_logw)
        return grammar_grad<false>(who, true, logits, lens, t, b, v, canon, g_state_off, g_arc_off, g, arc_src, arc_cls, arc_dst, accept, {},
                                   max_states, max_arcs, which, weights, out_logp, dlogits, workspace, workspace_bytes, stream);
    return grammar_grad<true>(who, true, logits, lens, t, b, v, canon, g_state_off, g_arc_off, g, arc_src, arc_cls, arc_dst, accept,
                              {arc_logw, final_logw, accept}, max_states, max_arcs, which, weights, out_logp, dlogits, workspace,
                              workspace_bytes, stream);
}
