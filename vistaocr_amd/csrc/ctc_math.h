// The log-space arithmetic every CTC kernel shares (loss, beam searches, alignment, edit scores, keyword search): one definition of
// each, so that two kernels that promise the same bits for the same sum really evaluate the same expression.
#pragma once
#include "vocr_common.h"

namespace {

constexpr float NEG_INF = -INFINITY;
constexpr int VMAX = 256;                    // columns of a row, in every kernel with symbol classes

// The class of column v under canon[V] (NULL: every column its own class): an entry that is not a canonical index <= v stands for
// itself.  The one statement of the rule, for the beam searches, the labelling scorers and the edit statistics.
__device__ __forceinline__ int class_of(const int32_t* __restrict__ canon, int v) {
    if (!canon) return v;
    int c = canon[v];
    if (c < 0 || c > v || canon[c] != c) c = v;
    return c;
}

// max-shifted log-sum-exp of two / three terms; all -inf stays -inf (never NaN)
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return logf(expf(a - m) + expf(b - m)) + m;
}

__device__ __forceinline__ float lse3(float a, float b, float c) {
    float m = fmaxf(a, fmaxf(b, c));
    if (m == NEG_INF) return NEG_INF;
    return logf(expf(a - m) + expf(b - m) + expf(c - m)) + m;
}

// a logsumexp kept as (max, sum): one exponential per term
struct LseAcc {
    float m = NEG_INF, s = 0.f;
    __device__ __forceinline__ void add(float v) {
        if (v == NEG_INF) return;
        const float e = expf(-fabsf(m - v));                     // m = -inf: 0
        s = v > m ? s * e + 1.f : s + e;
        m = fmaxf(m, v);
    }
    __device__ __forceinline__ float get() const { return m == NEG_INF ? NEG_INF : m + logf(s); }
};

}  // namespace
