// What the scorers of a KNOWN labelling share (the alignment ctc_align.hip, the edit scores ctc_edit.hip, the n-best gradient
// ctc_nbest.hip): the sweep over the extended sequence, ext[0..S), S = 2L+1, of the recursion
//   row_t(s) = lp_t(ext[s]) + lse3(row_(t-1)(s), row_(t-1)(s-1), row_(t-1)(s-2) iff ext[s] is a label whose class differs from ext[s-2]'s)
// in both of its row layouts, the lattice kernel built on it (edit scores, n-best gradient: both read and report the same bits for
// ln P_ctc(labels | x)), and the host side in front of every such call (shape limits, argument checks, LDS size).  The alignment keeps
// its own copy of the sweep with the Viterbi row beside the sum row (ctc_align.hip says why) and shares the constants and the host side.
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
// frames per position.
template <bool STORED>
struct SweepMap {
    int dir, len, S, L, T;
    float* dst;
    __device__ __forceinline__ int label(const int32_t* lab, int p) const { return (STORED && dir) ? lab[L - 1 - p] : lab[p]; }
    __device__ __forceinline__ int frame(int t) const { return (STORED && dir) ? len - 1 - t : t; }
    __device__ __forceinline__ int pos(int s) const { return (STORED && dir) ? S - 1 - s : s; }
};

// the two end states of the row after the last frame: positions S-1 and S-2 (-inf where there is none)
struct SweepEnd {
    float as, cs;
};

// One wave sweeps the len >= 1 frames of one labelling of S = 2L+1 <= SP positions.  lpb[t * tstride + v]: the line's class
// log-probabilities.  rows: sweep_floats(SP, 1) floats, read only when S > 64.
template <bool STORED>
__device__ __forceinline__ SweepEnd ctc_label_sweep(const float* __restrict__ lpb, long tstride, const int32_t* __restrict__ canon,
                                                    const int32_t* __restrict__ lab, int len, int S, int SP, float* rows,
                                                    const SweepMap<STORED>& map, int lane) {
    SweepEnd end;
    if (S <= 64) {
        const bool in = lane < S;
        const int e = (in && (lane & 1)) ? map.label(lab, lane >> 1) : 0;
        const int c = class_of(canon, e);
        const int c_m2 = __shfl_up(c, 2, 64);
        const bool skip = lane >= 2 && e != 0 && c != c_m2;
        const float* col = lpb + e;
        float* out = STORED ? map.dst + (long)map.pos(in ? lane : 0) * map.T : nullptr;
        float vs = NEG_INF;
        if (lane == 0 || (lane == 1 && S > 1)) vs = col[(long)map.frame(0) * tstride];
        if (STORED && in) out[map.frame(0)] = vs;
        float buf[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) buf[k] = col[(long)map.frame(min(1 + k, len - 1)) * tstride];
        for (int t0 = 1; t0 < len; t0 += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const int t = t0 + k;
                if (t < len) {                                   // wave-uniform
                    const float lpe = buf[k];
                    buf[k] = col[(long)map.frame(min(t + PF, len - 1)) * tstride];
                    float a2 = __shfl_up(vs, 1, 64), a3 = __shfl_up(vs, 2, 64);
                    if (lane < 1) a2 = NEG_INF;
                    if (!skip) a3 = NEG_INF;
                    vs = in ? lse3(vs, a2, a3) + lpe : NEG_INF;
                    if (STORED && in) out[map.frame(t)] = vs;
                }
            }
        }
        end.as = __shfl(vs, S - 1, 64);
        end.cs = S > 1 ? __shfl(vs, S - 2, 64) : NEG_INF;
    } else {
        float* rs = rows;                                        // rs[2 + s]
        int* ext = (int*)(rows + SP + 2);                        // label | class << 16
        float* em = rows + SP + 2 + SP;                          // em[k * SP + s]
        const int NC = (S + 63) >> 6;
        for (int s = lane; s < S; s += 64) {
            const int e = (s & 1) ? map.label(lab, s >> 1) : 0;
            ext[s] = e | (class_of(canon, e) << 16);
            const float v = s < 2 ? lpb[(long)map.frame(0) * tstride + e] : NEG_INF;
            rs[2 + s] = v;
            if (STORED) map.dst[(long)map.pos(s) * map.T + map.frame(0)] = v;
        }
        if (lane < 2) rs[lane] = NEG_INF;
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
                    float ns = NEG_INF;
                    if (in) {
                        const int x = ext[s];
                        const bool skip = s >= 2 && (x & 0xffff) != 0 && (x >> 16) != (ext[s - 2] >> 16);
                        ns = lse3(rs[2 + s], rs[1 + s], skip ? rs[s] : NEG_INF) + em[k * SP + s];
                    }
                    __builtin_amdgcn_wave_barrier();             // every lane of the chunk has read before any writes
                    if (in) {
                        rs[2 + s] = ns;
                        if (STORED) map.dst[(long)map.pos(s) * map.T + ft] = ns;
                    }
                }
                __syncthreads();
            }
        }
        end.as = rs[2 + S - 1];
        end.cs = rs[2 + S - 2];
    }
    return end;
}

// LATTICE: grid.x = B * n * 2 (direction fastest), 64 threads: alpha and beta of every (line, hypothesis) to
// lat: [B * n][2][SM = 2 * max_label_len + 1][T] floats, and ln P_ctc(labels | x) from the forward wave.
// !LATTICE: scores only - grid.x = B * n, the forward wave alone, nothing written to lat.
// Dynamic LDS (S > 64 only): sweep_floats(SP, 1) floats.
template <bool LATTICE>
__global__ __launch_bounds__(64) void ctc_lattice_kernel(const float* __restrict__ clp, const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ canon, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ label_lens, int T, int B, int V, int n,
                                                         int label_stride, int max_label_len, int SP, float* __restrict__ lat,
                                                         float* __restrict__ out_ctc) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x;
    const int prob = LATTICE ? blockIdx.x >> 1 : blockIdx.x, dir = LATTICE ? blockIdx.x & 1 : 0, b = prob / n;
    const int len = min(max(lens[b], 0), T);
    const int L = label_lens[prob];
    const int32_t* lab = labels + (long)prob * label_stride;
    const bool bad = labelling_bad(canon, lab, L, V, max_label_len, lane);
    if (bad || len == 0) {                                      // nobody reads a lattice of such a problem
        if (dir == 0 && lane == 0) out_ctc[prob] = (!bad && L == 0) ? 0.f : NEG_INF;
        return;
    }
    const int S = 2 * L + 1;
    const SweepMap<LATTICE> map = {dir, len, S, L, T, LATTICE ? lat + ((long)prob * 2 + dir) * (2 * max_label_len + 1) * T : nullptr};
    const SweepEnd end = ctc_label_sweep(clp + (long)b * V, (long)B * V, canon, lab, len, S, SP, sm, map, lane);
    if (dir == 0 && lane == 0) out_ctc[prob] = lse2(end.as, end.cs);
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

// what a call of the lattice kernel needs
constexpr size_t LATTICE_BYTES_MAX = (size_t)1 << 31;

struct LatticePlan {
    int sp;                // extended positions rounded up to 64
    size_t lds;            // dynamic LDS of the lattice kernel (0 when every labelling fits one wave)
    size_t lattice_bytes;  // alpha and beta of every (line, hypothesis)
    bool ok;
};

inline LatticePlan lattice_plan(int t, int b, int v, int n, int max_label_len) {
    LatticePlan p = {0, 0, 0, false};
    const LabelPlan lp = label_plan(t, b, v, n, max_label_len);
    if (!lp.ok) return p;
    p.sp = lp.sp;
    p.lds = sweep_floats(p.sp, 1) * 4;
    p.lattice_bytes = (size_t)b * n * 2 * (2 * (size_t)max_label_len + 1) * t * sizeof(float);
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
