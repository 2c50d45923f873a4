// What the scorers of a KNOWN labelling share (the alignment ctc_align.hip, the edit scores ctc_edit.hip, the n-best gradient
// ctc_nbest.hip, the alignment entropy ctc_entropy.hip): the sweep over the extended sequence, ext[0..S), S = 2L+1, of the recursion
//   cell_t(s) = step(cell_(t-1)(s), cell_(t-1)(s-1), cell_(t-1)(s-2) iff ext[s] is a label whose class differs from ext[s-2]'s, lp_t(ext[s]))
// over a CELL type (SumCell below: step = lp + lse3, the plain sum; EntCell of ctc_entropy.hip: the sum and an entropy beside it) in
// both of its row layouts, the lattice kernel built on it (edit scores, n-best gradient, entropy: all three report the same bits for
// ln P_ctc(labels | x)), the row pass that ends the two gradient kernels, and the host side in front of every such call (shape limits,
// argument checks, LDS size).  The alignment keeps its own copy of the sweep with the Viterbi row beside the sum row (ctc_align.hip says
// why) and shares the constants and the host side.
//   S <= 64 : one extended position per lane, the previous row in registers, neighbours by wave shuffles, the frame's gathered
//             class log-probability (which does not depend on the recursion) prefetched PF frames ahead.  No row in memory, no barrier.
//   S  > 64 : the row in memory (LDS, or the workspace where it no longer fits) with 2 leading -inf pads, ext[s] = label | class << 16
//             behind it, lanes over 64-position chunks updated in place from the highest chunk down (a chunk reads only positions that no
//             earlier chunk of the step wrote); the gathered log-probabilities of TB frames are staged in one pass of independent loads,
//             so the L2 round trip is paid once per TB frames.
#pragma once
#include "ctc_align_common.h"

namespace {

constexpr int PF = 8;                        // frames of loads in flight (the sweep at S <= 64; the edit scores' kernel 3)
constexpr int TB = 8;                        // the sweep at S > 64: frames staged per gather pass
constexpr size_t LDS_BUDGET = 144 * 1024;    // of the 160 KiB per CU

// floats of the S > 64 layout for sp = the longest S rounded up to 64: `rows` rows of sp + 2, ext[sp], the staged log-probabilities
// [TB][sp]; 0 when every labelling fits one wave.  The one size, for the LDS and for rows kept in a workspace.
__host__ __device__ constexpr size_t sweep_floats(int sp, int rows) {
    return sp <= 64 ? 0 : (size_t)rows * (sp + 2) + sp + (size_t)TB * sp;
}

// Which way a sweep runs and what it keeps.  STORED = false: forward, nothing stored (the members are not read).  STORED = true:
// direction dir = 0 forward, 1 backward - beta is alpha of the reversed labelling over the reversed frames, so position s' of the
// reversed labelling at reversed frame t' is position S-1-s' at frame len-1-t' - and every cell goes to dst TRANSPOSED, [s][t] with T
// frames per position, row r of the cell `plane` floats behind row r - 1.
template <bool STORED>
struct SweepMap {
    int dir, len, S, L, T;
    long plane;
    float* dst;
    __device__ __forceinline__ int label(const int32_t* lab, int p) const { return (STORED && dir) ? lab[L - 1 - p] : lab[p]; }
    __device__ __forceinline__ int frame(int t) const { return (STORED && dir) ? len - 1 - t : t; }
    __device__ __forceinline__ int pos(int s) const { return (STORED && dir) ? S - 1 - s : s; }
};

// A CELL is what the sweep keeps per (frame, extended position): ROWS floats, and how three predecessors and the frame's class
// log-probability u make the next one.  A cell type gives
//   none()                 the cell of no path            first(u)       the cell of a path that starts here, at frame 0
//   step(p1, p2, p3, u)    the recursion                   kill()         turns a predecessor into none() as far as step() looks
//   up(d), from(l)         the wave shuffles               get(p, stride, i), put(p, stride, i)   row r of the cell at p[r * stride + i]
//   finish(as, cs, ..)     the line's outputs from the two end cells (ENTROPY: there is a second one, 0 for a line without a sweep)
// SumCell is the plain sum; ctc_entropy.hip adds the (a, e) cell of the alignment entropy.
struct SumCell {
    static constexpr int ROWS = 1;
    static constexpr bool ENTROPY = false;                       // no second output
    float a;                                                     // ln of the mass of the partial paths that end here
    static __device__ __forceinline__ SumCell none() { return {NEG_INF}; }
    static __device__ __forceinline__ SumCell first(float u) { return {u}; }
    static __device__ __forceinline__ SumCell step(SumCell p1, SumCell p2, SumCell p3, float u) { return {lse3(p1.a, p2.a, p3.a) + u}; }
    __device__ __forceinline__ void kill() { a = NEG_INF; }
    __device__ __forceinline__ SumCell up(int d) const { return {__shfl_up(a, d, 64)}; }
    __device__ __forceinline__ SumCell from(int l) const { return {__shfl(a, l, 64)}; }
    static __device__ __forceinline__ SumCell get(const float* p, long, long i) { return {p[i]}; }
    __device__ __forceinline__ void put(float* p, long, long i) const { p[i] = a; }
    // ln P_ctc(labels | x) of problem i; the sum has no second output
    static __device__ __forceinline__ void finish(SumCell as, SumCell cs, float* out_ctc, float*, int i) { out_ctc[i] = lse2(as.a, cs.a); }
};

// the two end states of the row after the last frame: positions S-1 and S-2 (none() where there is none)
template <class Cell>
struct SweepEnd {
    Cell as, cs;
};

// One wave sweeps the len >= 1 frames of one labelling of S = 2L+1 <= SP positions.  lpb[t * tstride + v]: the line's class
// log-probabilities.  rows: sweep_floats(SP, Cell::ROWS) floats, read only when S > 64: row r of position s at
// rows[r * (SP + 2) + 2 + s], ext behind the last row, the staged frames behind ext.  STORED: row r of every cell goes to
// map.dst + r * map.plane.
template <class Cell, bool STORED>
__device__ __forceinline__ SweepEnd<Cell> ctc_label_sweep(const float* __restrict__ lpb, long tstride, const int32_t* __restrict__ canon,
                                                          const int32_t* __restrict__ lab, int len, int S, int SP, float* rows,
                                                          const SweepMap<STORED>& map, int lane) {
    SweepEnd<Cell> end;
    if (S <= 64) {
        const bool in = lane < S;
        const int e = (in && (lane & 1)) ? map.label(lab, lane >> 1) : 0;
        const int c = class_of(canon, e);
        const int c_m2 = __shfl_up(c, 2, 64);
        const bool skip = lane >= 2 && e != 0 && c != c_m2;
        const float* col = lpb + e;
        float* out = STORED ? map.dst + (long)map.pos(in ? lane : 0) * map.T : nullptr;
        Cell vs = Cell::none();
        if (lane == 0 || (lane == 1 && S > 1)) vs = Cell::first(col[(long)map.frame(0) * tstride]);
        if (STORED && in) vs.put(out, map.plane, map.frame(0));
        float buf[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) buf[k] = col[(long)map.frame(min(1 + k, len - 1)) * tstride];
        for (int t0 = 1; t0 < len; t0 += PF) {
            Cell kept[PF];                                       // STORED: the group's cells, stored behind its last step
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const int t = t0 + k;
                if (t < len) {                                   // wave-uniform
                    const float lpe = buf[k];
                    buf[k] = col[(long)map.frame(min(t + PF, len - 1)) * tstride];
                    Cell p2 = vs.up(1), p3 = vs.up(2);
                    if (lane < 1) p2.kill();
                    if (!skip) p3.kill();
                    // every lane steps, without a select on the recursion's path: a lane past S holds the blank's column and what
                    // nobody reads - the shuffles only look at lower lanes, the stores and the end cells only at lanes < S
                    vs = Cell::step(vs, p2, p3, lpe);
                    if (STORED) kept[k] = vs;
                }
            }
            // loads and stores share one counter, which can only be waited to zero while both are in flight: a store in every step
            // would make every step wait for the prefetched loads and for its own store
            if (STORED && in) {
#pragma unroll
                for (int k = 0; k < PF; ++k)
                    if (t0 + k < len) kept[k].put(out, map.plane, map.frame(t0 + k));
            }
        }
        end.as = vs.from(S - 1);
        end.cs = S > 1 ? vs.from(S - 2) : Cell::none();
    } else {
        const long pitch = SP + 2;
        float* rs = rows;                                        // rs[r * pitch + 2 + s]
        int* ext = (int*)(rows + Cell::ROWS * pitch);            // label | class << 16
        float* em = rows + Cell::ROWS * pitch + SP;              // em[k * SP + s]
        const int NC = (S + 63) >> 6;
        for (int s = lane; s < S; s += 64) {
            const int e = (s & 1) ? map.label(lab, s >> 1) : 0;
            ext[s] = e | (class_of(canon, e) << 16);
            Cell v = Cell::none();
            if (s < 2) v = Cell::first(lpb[(long)map.frame(0) * tstride + e]);
            v.put(rs, pitch, 2 + s);
            if (STORED) v.put(map.dst, map.plane, (long)map.pos(s) * map.T + map.frame(0));
        }
        if (lane < 2) Cell::none().put(rs, pitch, lane);
        __syncthreads();
        for (int t0 = 1; t0 < len; t0 += TB) {
            const int nk = min(TB, len - t0);
            for (int s = lane; s < S; s += 64) {
                const float* col = lpb + (ext[s] & 0xffff);
#pragma unroll
                for (int k = 0; k < TB; ++k)
                    if (k < nk) em[k * SP + s] = col[(long)map.frame(t0 + k) * tstride];
            }
            __syncthreads();
            for (int k = 0; k < nk; ++k) {
                const int ft = map.frame(t0 + k);
                for (int ch = NC - 1; ch >= 0; --ch) {
                    const int s = ch * 64 + lane;
                    const bool in = s < S;
                    Cell ns = Cell::none();
                    if (in) {
                        const int x = ext[s];
                        const bool skip = s >= 2 && (x & 0xffff) != 0 && (x >> 16) != (ext[s - 2] >> 16);
                        Cell p3 = Cell::get(rs, pitch, s);
                        if (!skip) p3.kill();
                        ns = Cell::step(Cell::get(rs, pitch, 2 + s), Cell::get(rs, pitch, 1 + s), p3, em[k * SP + s]);
                    }
                    __builtin_amdgcn_wave_barrier();             // every lane of the chunk has read before any writes
                    if (in) {
                        ns.put(rs, pitch, 2 + s);
                        if (STORED) ns.put(map.dst, map.plane, (long)map.pos(s) * map.T + ft);
                    }
                }
                __syncthreads();
            }
        }
        end.as = Cell::get(rs, pitch, 2 + S - 1);
        end.cs = Cell::get(rs, pitch, 2 + S - 2);
    }
    return end;
}

// LATTICE: grid.x = B * n * 2 (direction fastest), 64 threads: the forward and the backward cells of every (line, hypothesis) to
// lat: [B * n][2 directions][Cell::ROWS][SM = 2 * max_label_len + 1][T] floats, and the line's outputs (Cell::finish) from the forward
// wave.  !LATTICE: outputs only - grid.x = B * n, the forward wave alone, nothing written to lat.
// out_entropy: read only for a cell with ENTROPY, the second output.  Dynamic LDS (S > 64 only): sweep_floats(SP, Cell::ROWS) floats.
template <class Cell, bool LATTICE>
__global__ __launch_bounds__(64) void ctc_lattice_kernel(const float* __restrict__ clp, const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ canon, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ label_lens, int T, int B, int V, int n,
                                                         int label_stride, int max_label_len, int SP, float* __restrict__ lat,
                                                         float* __restrict__ out_ctc, float* __restrict__ out_entropy) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x;
    const int prob = LATTICE ? blockIdx.x >> 1 : blockIdx.x, dir = LATTICE ? blockIdx.x & 1 : 0, b = prob / n;
    const int len = min(max(lens[b], 0), T);
    const int L = label_lens[prob];
    const int32_t* lab = labels + (long)prob * label_stride;
    const bool bad = labelling_bad(canon, lab, L, V, max_label_len, lane);
    if (bad || len == 0) {                                      // nobody reads a lattice of such a problem
        if (dir == 0 && lane == 0) {
            out_ctc[prob] = (!bad && L == 0) ? 0.f : NEG_INF;
            if (Cell::ENTROPY) out_entropy[prob] = 0.f;
        }
        return;
    }
    const int S = 2 * L + 1;
    const long plane = (2 * (long)max_label_len + 1) * T;
    const SweepMap<LATTICE> map = {dir, len, S, L, T, plane, LATTICE ? lat + ((long)prob * 2 + dir) * Cell::ROWS * plane : nullptr};
    const SweepEnd<Cell> end = ctc_label_sweep<Cell>(clp + (long)b * V, (long)B * V, canon, lab, len, S, SP, sm, map, lane);
    if (dir == 0 && lane == 0) Cell::finish(end.as, end.cs, out_ctc, out_entropy, prob);
}

constexpr int TT = 16;                       // the gradient kernels: frames per workgroup
constexpr int NG = 4;                        // the gradient kernels: groups of TT lanes (TT * NG = 64), each with accumulators of its own

// The row pass of a gradient kernel (n-best, entropy), after its lanes have filled acc[NG][V][TT] with the class sums of the tile
// of TT frames at t0 of line b: frame by frame the lanes stride over the row's columns - the row's log-softmax again (wave_row_lse, the
// function class_logprob_rows_kernel calls: with no classes the member share is exactly 1), the NG partial sums added in order, one
// coalesced store of share * G - p_t(v) * w.  Frames from `live` on (the line's length, or 0 for a line written as zeros) are zeros.
__device__ __forceinline__ void ctc_grad_rows(const float* __restrict__ logits, const float* __restrict__ clp,
                                              const int32_t* __restrict__ canon, const float* acc, int T, int B, int V, int b, int t0,
                                              int live, float w, float* __restrict__ dlogits, int lane) {
    for (int kk = 0; kk < TT; ++kk) {
        const int tr = t0 + kk;
        if (tr >= T) break;
        const long row = (long)tr * B + b;
        float* out = dlogits + row * V;
        if (tr >= live) {
            for (int v = lane; v < V; v += 64) out[v] = 0.f;
            continue;
        }
        const float* xr = logits + row * V;
        const float* cr = clp + row * V;
        const RowLse rl = wave_row_lse(xr, V, lane);
        for (int v = lane; v < V; v += 64) {
            const float lpv = row_logprob(rl, xr, v);
            const float* a = acc + (long)class_of(canon, v) * TT + kk;
            float G = a[0];
#pragma unroll
            for (int j = 1; j < NG; ++j) G += a[(long)j * V * TT];
            const float share = (lpv == NEG_INF) ? 0.f : expf(lpv - cr[v]);     // p_t(v) / P_t(class(v))
            out[v] = share * G - expf(lpv) * w;
        }
    }
}

// ---- the host side in front of vocr_ctc_align, vocr_ctc_edit_scores and vocr_ctc_nbest_grad

struct LabelPlan {
    int sp;                // extended positions rounded up to 64
    bool ok;               // within the limits every labelling entry shares
};

inline LabelPlan label_plan(int t, int b, int v, int n, int max_label_len) {
    LabelPlan p = {0, false};
    if (t <= 0 || b <= 0 || v <= 1 || v > VMAX || n < 1 || n > NMAX || max_label_len < 0 || max_label_len > t) return p;
    if ((long)t * b * n >= (1L << 31)) return p;
    p.sp = ((2 * max_label_len + 1 + 63) / 64) * 64;
    p.ok = true;
    return p;
}

// what a call of the lattice kernel needs for a cell of `rows` floats
constexpr size_t LATTICE_BYTES_MAX = (size_t)1 << 31;

struct LatticePlan {
    int sp;                // extended positions rounded up to 64
    size_t lds;            // dynamic LDS of the lattice kernel (0 when every labelling fits one wave)
    size_t lattice_bytes;  // the forward and the backward cells of every (line, hypothesis)
    bool ok;
};

inline LatticePlan lattice_plan(int t, int b, int v, int n, int max_label_len, int rows) {
    LatticePlan p = {0, 0, 0, false};
    const LabelPlan lp = label_plan(t, b, v, n, max_label_len);
    if (!lp.ok) return p;
    p.sp = lp.sp;
    p.lds = sweep_floats(p.sp, rows) * 4;
    p.lattice_bytes = (size_t)b * n * 2 * rows * (2 * (size_t)max_label_len + 1) * t * sizeof(float);
    p.ok = p.lds <= LDS_BUDGET && p.lattice_bytes <= LATTICE_BYTES_MAX;
    return p;
}

// the shape checks of a labelling entry `who`, behind its null-pointer check (each entry has its own list of pointers)
inline int check_labelling_shape(const char* who, int t, int b, int v, int n, int label_stride, int max_label_len) {
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 1 && v <= VMAX, "%s: need t > 0, b > 0, 2 <= v <= %d (t=%d b=%d v=%d)", who, VMAX, t, b, v);
    VOCR_CHECK_ARG(n >= 1 && n <= NMAX, "%s: need 1 <= n <= %d (n=%d)", who, NMAX, n);
    VOCR_CHECK_ARG(max_label_len >= 0 && max_label_len <= t && label_stride >= max_label_len,
                   "%s: need 0 <= max_label_len <= t and label_stride >= max_label_len (max_label_len=%d t=%d label_stride=%d)", who,
                   max_label_len, t, label_stride);
    return VOCR_OK;
}

}  // namespace
