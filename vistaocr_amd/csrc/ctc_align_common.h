// What the CTC alignment (ctc_align.hip) and the CTC edit scores (ctc_edit.hip) share: the class rule of the beam searches and the
// class log-probability pass, so that both read the same bits for a (frame, column).
#pragma once
#include "ctc_math.h"

namespace {

constexpr int VMAX = 256;                    // as vocr_ctc_beam_search
constexpr int NMAX = 128;

// canon sanitised as in the beam searches: an entry that is not a canonical index <= v stands for itself
__device__ __forceinline__ int class_of(const int32_t* __restrict__ canon, int v) {
    if (!canon) return v;
    int c = canon[v];
    if (c < 0 || c > v || canon[c] != c) c = v;
    return c;
}

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
        float m = NEG_INF;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, xr[v]);
        m = wave_max(m);
        float s = 0.f;
        if (m != NEG_INF)
            for (int v = lane; v < V; v += 64) s += expf(xr[v] - m);
        s = wave_sum(s);
        const float lse = m + logf(s);
        __builtin_amdgcn_wave_barrier();                          // the previous row's readers are done with rw
        for (int v = lane; v < V; v += 64) rw[v] = (m == NEG_INF) ? NEG_INF : xr[v] - lse;      // a row of -inf stays -inf, never NaN
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

}  // namespace
