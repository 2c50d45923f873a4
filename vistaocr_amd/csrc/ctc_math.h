// The log-space arithmetic every CTC kernel shares (loss, beam searches, alignment, edit scores, keyword search): one definition of
// each, so that two kernels that promise the same bits for the same sum really evaluate the same expression.
#pragma once
#include "vocr_common.h"

namespace {

constexpr float NEG_INF = -INFINITY;

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
