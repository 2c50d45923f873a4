// What the kernels that score a labelling or a query against a line's logits share (ctc_align.hip, ctc_edit.hip, ctc_nbest.hip through
// ctc_lattice.h; ctc_keyword.hip; the class rule also serves edit_distance.hip): the check of a labelling, the wave-per-row log-softmax
// and the class log-probability pass in front of every workspace, so that all of them read the same bits for a (frame, column).
#pragma once
#include "ctc_math.h"

namespace {

constexpr int NMAX = 128;

// a labelling that cannot be scored: bad length, a label outside (0, V) or in the blank's class.  Wave-uniform.
__device__ __forceinline__ bool labelling_bad(const int32_t* __restrict__ canon, const int32_t* __restrict__ lab, int L, int V,
                                              int max_label_len, int lane) {
    if (L < 0 || L > max_label_len) return true;
    bool mine = false;
    for (int p = lane; p < L; p += 64) {
        const int v = lab[p];
        mine |= (v <= 0 || v >= V) || class_of(canon, min(max(v, 0), V - 1)) == 0;
    }
    return __any(mine);
}

// The log-softmax of one row of V logits by one wave: the row's maximum m and lse = m + ln sum exp(x - m), so that column v's
// log-probability is row_logprob(r, x, v).  A row of -inf stays -inf, never NaN.  The one definition: a kernel that needs the bits of
// class_logprob_rows_kernel's log-softmax again (the n-best gradient) calls these.
struct RowLse {
    float m, lse;
};

__device__ __forceinline__ RowLse wave_row_lse(const float* __restrict__ xr, int V, int lane) {
    float m = NEG_INF;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, xr[v]);
    m = wave_max(m);
    float s = 0.f;
    if (m != NEG_INF)
        for (int v = lane; v < V; v += 64) s += expf(xr[v] - m);
    s = wave_sum(s);
    return {m, m + logf(s)};
}

__device__ __forceinline__ float row_logprob(const RowLse& r, const float* xr, int v) { return (r.m == NEG_INF) ? NEG_INF : xr[v] - r.lse; }

// 16 rows per block, one wave per row at a time.  clp[row][v] = ln P(class of v | frame); rows with t >= lens[b] are never read and not
// written.  Only columns whose class has more than one member pay for the logsumexp over the members.
constexpr int ROWS_PER_BLOCK = 16;

__global__ __launch_bounds__(256) void class_logprob_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens,
                                                                 const int32_t* __restrict__ canon, float* __restrict__ clp, int T, int B,
                                                                 int V) {
    __shared__ int s_cls[VMAX];
    __shared__ int s_multi[VMAX];
    __shared__ float s_row[4][VMAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < V) s_cls[tid] = class_of(canon, tid);
    __syncthreads();
    if (tid < V) {
        int members = 0;
        if (canon)
            for (int w = 0; w < V; ++w) members += s_cls[w] == s_cls[tid] ? 1 : 0;
        s_multi[tid] = members > 1;
    }
    __syncthreads();
    float* rw = s_row[wave];
    for (int r = wave; r < ROWS_PER_BLOCK; r += 4) {
        const int row = blockIdx.x * ROWS_PER_BLOCK + r;
        if (row >= T * B) break;
        const int t = row / B, b = row - t * B;
        if (t >= min(max(lens[b], 0), T)) continue;
        const float* xr = x + (long)row * V;
        const RowLse rl = wave_row_lse(xr, V, lane);
        __builtin_amdgcn_wave_barrier();                          // the previous row's readers are done with rw
        for (int v = lane; v < V; v += 64) rw[v] = row_logprob(rl, xr, v);
        __builtin_amdgcn_wave_barrier();
        float* out = clp + (long)row * V;
        for (int v = lane; v < V; v += 64) {
            float lp = rw[v];
            if (s_multi[v]) {
                const int c = s_cls[v];
                float mm = NEG_INF;
                for (int w = c; w < V; ++w)
                    if (s_cls[w] == c) mm = fmaxf(mm, rw[w]);
                lp = NEG_INF;
                if (mm != NEG_INF) {
                    float ss = 0.f;
                    for (int w = c; w < V; ++w)
                        if (s_cls[w] == c) ss += expf(rw[w] - mm);
                    lp = mm + logf(ss);
                }
            }
            out[v] = lp;
        }
    }
}

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// the class log-probabilities in front of a workspace, rounded so that 16-byte words behind them stay aligned
inline size_t clp_bytes(int t, int b, int v) { return align16((size_t)t * b * v * sizeof(float)); }

// ... and their launch, under the entry's name `who`
inline int launch_class_logprob(const char* who, const float* logits, const int32_t* lens, const int32_t* canon, float* clp, int t, int b,
                                int v, hipStream_t s) {
    class_logprob_rows_kernel<<<vocr_cdiv((long)t * b, ROWS_PER_BLOCK), 256, 0, s>>>(logits, lens, canon, clp, t, b, v);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        vocr_set_error("%s(class_logprob): launch failed: %s", who, hipGetErrorString(e));
        return VOCR_ELAUNCH;
    }
    return VOCR_OK;
}

}  // namespace
