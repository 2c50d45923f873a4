// The CTC lattice kernel the edit scores (ctc_edit.hip) and the n-best gradient (ctc_nbest.hip) share: alpha and beta of every
// (line, hypothesis) written to a workspace, and ln P_ctc(labels | x) from the forward wave, so that both read and report the same bits.
#pragma once
#include "ctc_align_common.h"

namespace {

constexpr int PF = 8;                        // frames of loads in flight (kernel 2, S <= 64; kernel 3)
constexpr int TB = 8;                        // kernel 2, S > 64: frames staged per gather pass
constexpr size_t LDS_BUDGET = 144 * 1024;    // of the 160 KiB per CU

// LATTICE: grid.x = B * n * 2 (direction fastest), 64 threads.  lat: [B * n][2][SM = 2 * max_label_len + 1][T] floats.  Dynamic LDS (S > 64 only):
// the row with 2 leading -inf pads, ext[SP], the staged log-probabilities [TB][SP].
// !LATTICE: scores only - grid.x = B * n, the forward wave alone, the same expressions in the same order, nothing written to lat.
template <bool LATTICE>
__global__ __launch_bounds__(64) void ctc_edit_lattice_kernel(const float* __restrict__ clp, const int32_t* __restrict__ lens,
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
    const long tstride = (long)B * V;
    const float* lpb = clp + (long)b * V;                       // lpb[t * tstride + v]
    const bool bad = labelling_bad(canon, lab, L, V, max_label_len, lane);
    if (bad || len == 0) {                                      // kernel 3 reads no lattice of such a problem
        if (dir == 0 && lane == 0) out_ctc[prob] = (!bad && L == 0) ? 0.f : NEG_INF;
        return;
    }
    const int S = 2 * L + 1;
    float* dst = LATTICE ? lat + ((long)prob * 2 + dir) * (2 * max_label_len + 1) * T : nullptr;
    // backward: position s' of the reversed labelling at reversed frame t' is position S-1-s' at frame len-1-t'
#define LABEL_AT(p) (dir ? lab[L - 1 - (p)] : lab[(p)])
#define FRAME(t) (dir ? len - 1 - (t) : (t))
#define POS(s) (dir ? S - 1 - (s) : (s))
    float as, cs;                                               // the two end states of the last frame
    if (S <= 64) {
        const bool in = lane < S;
        const int e = (in && (lane & 1)) ? LABEL_AT(lane >> 1) : 0;
        const int c = class_of(canon, e);
        const int c_m2 = __shfl_up(c, 2, 64);
        const bool skip = lane >= 2 && e != 0 && c != c_m2;
        const float* col = lpb + e;
        float* out = LATTICE ? dst + (long)POS(in ? lane : 0) * T : nullptr;
        float vs = NEG_INF;
        if (lane == 0 || (lane == 1 && S > 1)) vs = col[(long)FRAME(0) * tstride];
        if (LATTICE && in) out[FRAME(0)] = vs;
        float buf[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) buf[k] = col[(long)FRAME(min(1 + k, len - 1)) * tstride];
        for (int t0 = 1; t0 < len; t0 += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const int t = t0 + k;
                if (t < len) {                                   // wave-uniform
                    const float lpe = buf[k];
                    buf[k] = col[(long)FRAME(min(t + PF, len - 1)) * tstride];
                    float a2 = __shfl_up(vs, 1, 64), a3 = __shfl_up(vs, 2, 64);
                    if (lane < 1) a2 = NEG_INF;
                    if (!skip) a3 = NEG_INF;
                    vs = in ? lse3(vs, a2, a3) + lpe : NEG_INF;
                    if (LATTICE && in) out[FRAME(t)] = vs;
                }
            }
        }
        as = __shfl(vs, S - 1, 64);
        cs = S > 1 ? __shfl(vs, S - 2, 64) : NEG_INF;
    } else {
        float* rs = sm;                                          // rs[2 + s]
        int* ext = (int*)(sm + SP + 2);                          // label | class << 16
        float* em = sm + SP + 2 + SP;                            // em[k * SP + s]
        const int NC = (S + 63) >> 6;
        for (int s = lane; s < S; s += 64) {
            const int e = (s & 1) ? LABEL_AT(s >> 1) : 0;
            ext[s] = e | (class_of(canon, e) << 16);
            const float v = s < 2 ? lpb[(long)FRAME(0) * tstride + e] : NEG_INF;
            rs[2 + s] = v;
            if (LATTICE) dst[(long)POS(s) * T + FRAME(0)] = v;
        }
        if (lane < 2) rs[lane] = NEG_INF;
        __syncthreads();
        for (int t0 = 1; t0 < len; t0 += TB) {
            const int nk = min(TB, len - t0);
            for (int s = lane; s < S; s += 64) {
                const float* col = lpb + (ext[s] & 0xffff);
#pragma unroll
                for (int k = 0; k < TB; ++k)
                    if (k < nk) em[k * SP + s] = col[(long)FRAME(t0 + k) * tstride];
            }
            __syncthreads();
            for (int k = 0; k < nk; ++k) {
                const int ft = FRAME(t0 + k);
                for (int ch = NC - 1; ch >= 0; --ch) {           // a chunk reads only positions that no earlier chunk of the step wrote
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
                        if (LATTICE) dst[(long)POS(s) * T + ft] = ns;
                    }
                }
                __syncthreads();
            }
        }
        as = rs[2 + S - 1];
        cs = rs[2 + S - 2];
    }
#undef LABEL_AT
#undef FRAME
#undef POS
    if (dir == 0 && lane == 0) out_ctc[prob] = lse2(as, cs);
}

}  // namespace
