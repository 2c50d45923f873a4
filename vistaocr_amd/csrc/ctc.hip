// CTC loss + gradient w.r.t. pre-softmax activations (stands in for warpctc_pytorch.CTCLoss, reference call
// sites src/train_cnn_lstm.py:358,138), greedy best-path decode (src/models/cnnlstm.py:479-541), and the
// fused gradient-clamp + Adam update (src/train_cnn_lstm.py:143-149,363).
//
// CTC: blank = 0, extended label l' of length S = 2L+1, log-space alpha/beta recursions in fp32 with the
// max-shifted log-sum-exp (the same formulation as the PyTorch-CPU criterion the parity target uses).
//   kernel 1  row-wise log-softmax            : one wave per (t,b) row
//   kernel 2  alpha and beta sweeps           : one wave per (sample, direction); lanes over s; the previous
//                                               row lives in registers (S <= 128) or in LDS
//   kernel 3  gradient                        : one wave per (t,b); lanes over the alphabet
#include "ctc_math.h"

namespace {

__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* __restrict__ x, float* __restrict__ lp,
                                                               int rows, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (long)row * V;
    float m = NEG_INF;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, xr[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(xr[v] - m);
    s = wave_sum(s);
    const float lse = m + logf(s);
    float* lr = lp + (long)row * V;
    for (int v = lane; v < V; v += 64) lr[v] = xr[v] - lse;
}

// Alpha and beta of one sample in one body: beta is alpha of the reversed labelling over the reversed frames, so the beta wave
// (blockIdx.x & 1) runs the alpha recursion in MIRRORED coordinates - position s' = S-1-s, frame t' = Tb-1-t, label lab[L-1-p'] - and
// stores every value to its un-mirrored place in ab[b][dir][t][s].  The mirror is folded into wave-uniform bases and signed strides
// computed once (a frame step of +-B*V in lp, a row step of +-SP in ab, a label step of +-1): the loops below have no direction
// select, and both directions evaluate the same expressions in the same order per element as a hand-written beta would (the
// neighbours s, s+1, s+2 of a beta step are s', s'-1, s'-2).  Columns s in [S, SP) of the rows t < Tb are written -inf by the lanes
// whose s' >= S (they keep the identity column s = s'); rows t >= Tb are never written.
struct Mirror {
    int S, Tb;
    int step, lab0, col0;      // +-1; the label under mirrored odd position s': lab[lab0 + step * (s' >> 1)]; the stored column of s' < S: col0 + step * s'
    long fstep, rstep;         // frame t' of a column of lp: lp0[t' * fstep]; row t' of ab: out[t' * rstep]
    const int32_t* lab;
    const float* lp0;
    float* out;
    __device__ __forceinline__ int ext(int s) const { return (s >= 0 && s < S && (s & 1)) ? lab[lab0 + step * (s >> 1)] : 0; }
    __device__ __forceinline__ int col(int s) const { return s < S ? col0 + step * s : s; }
};

__device__ __forceinline__ Mirror mirror_of(int b, int dirn, const float* __restrict__ lp, const int32_t* __restrict__ labels,
                                            const int32_t* __restrict__ label_offsets, const int32_t* __restrict__ label_lens,
                                            const int32_t* __restrict__ act_lens, float* __restrict__ ab, int T, int B, int V, int SP) {
    Mirror m;
    const int L = label_lens[b];
    m.S = 2 * L + 1;
    m.Tb = act_lens[b];
    m.lab = labels + label_offsets[b];
    m.step = dirn ? -1 : 1;
    m.lab0 = dirn ? L - 1 : 0;
    m.col0 = dirn ? m.S - 1 : 0;
    const long tstride = (long)B * V;
    const int t0 = dirn ? max(m.Tb - 1, 0) : 0;                    // the frame that t' = 0 stands for
    m.fstep = dirn ? -tstride : tstride;
    m.rstep = dirn ? -SP : SP;
    m.lp0 = lp + (long)t0 * tstride + (long)b * V;
    m.out = ab + ((long)(b * 2 + dirn) * T + t0) * SP;
    return m;
}

// grid.x = 2*B (even: alpha of sample b, odd: beta); 64 threads.  ab[b][dir][t][s], row pitch SP.  Any label length: lanes stride
// over s', the previous row lives in LDS.
__global__ __launch_bounds__(64) void ctc_alpha_beta_lds_kernel(const float* __restrict__ lp, const int32_t* __restrict__ labels,
                                                                const int32_t* __restrict__ label_offsets,
                                                                const int32_t* __restrict__ label_lens,
                                                                const int32_t* __restrict__ act_lens, float* __restrict__ ab,
                                                                float* __restrict__ nll, int T, int B, int V, int SP) {
    extern __shared__ float sm[];            // [2][SP+4] rows (row[2 + s'], with 2 leading -inf pads) + int ext[SP]
    const int b = blockIdx.x >> 1, dirn = blockIdx.x & 1;
    const int lane = threadIdx.x;
    const Mirror m = mirror_of(b, dirn, lp, labels, label_offsets, label_lens, act_lens, ab, T, B, V, SP);
    const int S = m.S, Tb = m.Tb;
    if (Tb <= 0) {
        if (dirn == 0 && lane == 0) nll[b] = (S == 1) ? 0.f : INFINITY;
        return;
    }
    float* prev = sm;
    float* cur = sm + (SP + 4);
    int* ext = (int*)(sm + 2 * (SP + 4));
    for (int s = lane; s < SP; s += 64) ext[s] = m.ext(s);
    for (int s = lane; s < SP + 4; s += 64) { prev[s] = NEG_INF; cur[s] = NEG_INF; }
    __syncthreads();
    for (int s = lane; s < SP; s += 64) {
        float v = NEG_INF;
        if (s == 0 || (s == 1 && S > 1)) v = m.lp0[ext[s]];
        prev[2 + s] = v;
        m.out[m.col(s)] = v;
    }
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        const float* lt = m.lp0 + t * m.fstep;
        float* ot = m.out + t * m.rstep;
        for (int s = lane; s < SP; s += 64) {
            float v = NEG_INF;
            if (s < S) {
                const int e = ext[s];
                const float a1 = prev[2 + s], a2 = prev[1 + s];
                const float a3 = (s >= 2 && e != 0 && e != ext[s - 2]) ? prev[s] : NEG_INF;
                const float l = lse3(a1, a2, a3);
                v = (l == NEG_INF) ? NEG_INF : l + lt[e];
            }
            cur[2 + s] = v;
            ot[m.col(s)] = v;
        }
        __syncthreads();
        float* tmp = prev; prev = cur; cur = tmp;
    }
    // -ln(alpha[S-1] + alpha[S-2]); S = 1: the second is a pad; +inf when neither end state is reachable
    if (dirn == 0 && lane == 0) nll[b] = -lse2(prev[2 + S - 1], prev[2 + S - 2]);
}

// The same sweeps for S = 2L+1 <= 64 * NP with NP extended-label positions per lane, s' = lane + 64 * j: the previous row stays in
// registers and neighbours are fetched with wave shuffles (no LDS, no barrier), and the one global operand of a step, lp[t][b][l'_s],
// does not depend on the recursion, so it is gathered PF steps ahead.  Same expressions in the same order per element as
// ctc_alpha_beta_lds_kernel: results are bit-identical.
//   NP = 1 (L <= 31: every BASELINE workload).  The LDS kernel paid an L2/HBM round trip per time step for the gather (0.73 us x 294
//          steps = 215 us on the critical path of every training step).
//   NP = 2 (32 <= L <= 63: the long lines of BASELINE configs[3], ~1200 px with W / 30 labels): the seam between the halves is crossed
//          with two broadcasts per step, lanes 0 and 1 of half j taking lanes 63 and 62 of half j-1.  The LDS kernel took 622 us for
//          T = 576 (1.08 us per frame, chip otherwise idle: the backward waits for it); this one 136 us.
template <int NP>
__global__ __launch_bounds__(64) void ctc_alpha_beta_reg_kernel(const float* __restrict__ lp, const int32_t* __restrict__ labels,
                                                                const int32_t* __restrict__ label_offsets,
                                                                const int32_t* __restrict__ label_lens,
                                                                const int32_t* __restrict__ act_lens, float* __restrict__ ab,
                                                                float* __restrict__ nll, int T, int B, int V) {
    constexpr int SP = 64 * NP, PF = 8;
    const int b = blockIdx.x >> 1, dirn = blockIdx.x & 1;
    const int lane = threadIdx.x;
    const Mirror m = mirror_of(b, dirn, lp, labels, label_offsets, label_lens, act_lens, ab, T, B, V, SP);
    const int S = m.S, Tb = m.Tb;
    if (Tb <= 0) {
        if (dirn == 0 && lane == 0) nll[b] = (S == 1) ? 0.f : INFINITY;
        return;
    }
    // per lane only 32-bit offsets: the label (its column of an lp row) and the stored column; the row bases are wave-uniform
    bool in[NP], skip[NP];
    unsigned e[NP], c[NP];
    float v[NP], buf[NP][PF];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int s = lane + 64 * j;
        e[j] = m.ext(s);
        c[j] = m.col(s);
        in[j] = s < S;
        skip[j] = s >= 2 && e[j] != 0 && e[j] != (unsigned)m.ext(s - 2);
        v[j] = (s == 0 || (s == 1 && S > 1)) ? m.lp0[e[j]] : NEG_INF;
        m.out[c[j]] = v[j];
#pragma unroll
        for (int k = 0; k < PF; ++k) buf[j][k] = (m.lp0 + min(1 + k, Tb - 1) * m.fstep)[e[j]];
    }
    for (int t0 = 1; t0 < Tb; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            if (t < Tb) {                                        // wave-uniform
                const float* ahead = m.lp0 + min(t + PF, Tb - 1) * m.fstep;
                float* ot = m.out + t * m.rstep;
                float lpe[NP], a2[NP], a3[NP];
#pragma unroll
                for (int j = 0; j < NP; ++j) {                   // every shuffle reads the old row, before any half is updated
                    lpe[j] = buf[j][k];
                    buf[j][k] = ahead[e[j]];
                    a2[j] = __shfl_up(v[j], 1, 64);
                    a3[j] = __shfl_up(v[j], 2, 64);
                    if (j == 0) {
                        if (lane < 1) a2[j] = NEG_INF;
                    } else {
                        const float w63 = __shfl(v[j > 0 ? j - 1 : 0], 63, 64), w62 = __shfl(v[j > 0 ? j - 1 : 0], 62, 64);
                        if (lane == 0) { a2[j] = w63; a3[j] = w62; }
                        if (lane == 1) a3[j] = w63;
                    }
                    if (!skip[j]) a3[j] = NEG_INF;
                }
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    const float l = lse3(v[j], a2[j], a3[j]);
                    v[j] = (in[j] && l != NEG_INF) ? l + lpe[j] : NEG_INF;
                    ot[c[j]] = v[j];
                }
            }
        }
    }
    if (dirn == 0) {
        // alpha[S-1], alpha[S-2]: either may sit in any half (a short line of a batch with long ones keeps both in the first)
        float a = NEG_INF, c = NEG_INF;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const float aj = __shfl(v[j], (S - 1) & 63, 64), cj = __shfl(v[j], (S - 2) & 63, 64);
            if ((S - 1) >> 6 == j) a = aj;
            if (S > 1 && (S - 2) >> 6 == j) c = cj;
        }
        if (lane == 0) nll[b] = -lse2(a, c);                     // +inf when neither end state is reachable
    }
}

// one wave per (t,b): grad[v] = exp(lp[v]) - exp(lse_{s: l'_s = v}(alpha+beta) + nll - lp[v]); zero for t >= act_len
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ lp, const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ label_offsets,
                                                       const int32_t* __restrict__ label_lens,
                                                       const int32_t* __restrict__ act_lens, const float* __restrict__ ab,
                                                       const float* __restrict__ nll, float* __restrict__ grad, int T, int B,
                                                       int V, int SP) {
    extern __shared__ float sm[];           // per wave: V floats (log-sum accumulators)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    float* accv = sm + wave * V;
    const bool valid = row < T * B;
    const int t = valid ? row / B : 0, b = valid ? row % B : 0;
    const int Tb = act_lens[b];
    const bool act = valid && t < Tb;
    float* g = grad + (long)row * V;
    const int L = label_lens[b], S = 2 * L + 1;
    const int32_t* lab = labels + label_offsets[b];
    const float* al = ab + ((long)(b * 2 + 0) * T + t) * SP;
    const float* be = ab + ((long)(b * 2 + 1) * T + t) * SP;
    const float* l = lp + (long)(valid ? row : 0) * V;
    if (act) {
        for (int v = lane; v < V; v += 64) accv[v] = NEG_INF;
    }
    __syncthreads();
    if (act) {
        // blanks (even s) all map to v = 0: reduce them across lanes
        float mb = NEG_INF;
        for (int s = 2 * lane; s < S; s += 128) mb = fmaxf(mb, al[s] + be[s]);
        mb = wave_max(mb);
        float sb = 0.f;
        if (mb != NEG_INF)
            for (int s = 2 * lane; s < S; s += 128) sb += expf(al[s] + be[s] - mb);
        sb = wave_sum(sb);
        // labels (odd s): lane 0 walks them in order; L is small (tens), duplicates stay exact and ordered
        if (lane == 0) {
            accv[0] = (mb == NEG_INF) ? NEG_INF : mb + logf(sb);
            for (int i = 0; i < L; ++i) {
                const int s = 2 * i + 1, v = lab[i];
                const float x = al[s] + be[s];
                const float cur = accv[v];
                const float m = fmaxf(cur, x);
                accv[v] = (m == NEG_INF) ? NEG_INF : m + logf(expf(cur - m) + expf(x - m));
            }
        }
    }
    __syncthreads();
    if (act) {
        const float nl = nll[b];
        for (int v = lane; v < V; v += 64) {
            const float lpv = l[v];
            const float a = accv[v];
            const float occ = (a == NEG_INF) ? 0.f : expf(a + nl - lpv);
            g[v] = expf(lpv) - occ;
        }
    } else if (valid) {
        for (int v = lane; v < V; v += 64) g[v] = 0.f;
    }
}

__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, int32_t* __restrict__ idx,
                                                          float* __restrict__ maxv, int rows, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (long)row * V;
    float m = NEG_INF;
    int mi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
        const float f = xr[v];
        if (mi == 0x7fffffff || f > m) { m = f; mi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(mi, o, 64);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }   // first maximum wins, like numpy.argmax
    }
    if (lane == 0) { idx[row] = mi; maxv[row] = m; }
}

// one thread per sample (T is a few hundred): blank / low-activation / repeat collapse of decode_without_lm
__global__ void greedy_collapse_kernel(const int32_t* __restrict__ idx, const float* __restrict__ maxv,
                                       const int32_t* __restrict__ lens, const int32_t* __restrict__ canon,
                                       int32_t* __restrict__ out_labels, int32_t* __restrict__ out_counts, int T, int B,
                                       float thresh) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int len = min(lens[b], T);
    int prev = -1, n = 0;
    for (int t = 0; t < len; ++t) {
        const int k = idx[(long)t * B + b];
        if (k == 0) { prev = -1; continue; }
        if (maxv[(long)t * B + b] < thresh) { prev = -1; continue; }
        const int ck = canon[k];
        if (ck == prev) continue;
        out_labels[(long)b * T + n++] = k;
        prev = ck;
    }
    out_counts[b] = n;
}

// NaN policy: grad.clamp_(-5, 5) of the reference propagates NaN (torch.clamp), so a NaN gradient must reach the
// weights and the next loss instead of being turned into a finite +-clamp update by fminf/fmaxf; the first NaN seen is
// also recorded in the caller's health word (health[1]) so the host can fail the step without an extra sync.
__device__ __forceinline__ float clamp_keep_nan(float x, float c) { return (x != x) ? x : fminf(fmaxf(x, -c), c); }

__global__ __launch_bounds__(256) void clamp_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                                                         float omb1, float beta2, float omb2, float eps, float wd, float clampv,
                                                         float gscale, float step_size, float bc2_sqrt, int32_t* health) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (; i < n; i += stride) {
        float gr = g[i] * gscale;
        bad |= (gr != gr);
        gr = clamp_keep_nan(gr, clampv);
        const float pv = p[i];
        if (wd != 0.f) gr = gr + wd * pv;
        const float mo = m[i];
        const float mi = mo + omb1 * (gr - mo);                     // exp_avg.lerp_(grad, 1-beta1)
        const float vi = v[i] * beta2 + omb2 * (gr * gr);           // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pv - step_size * (mi / denom);
    }
    if (health && bad) health[1] = 1;
}

// in-place elementwise clamp (the reference's `param.grad.data.clamp_(min=-5, max=5)` loop) for optimisers that are not
// FlatClampAdam; NaN stays NaN
__global__ void clamp_kernel(float* __restrict__ x, size_t n, float c, int vec, int32_t* health) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n4 = vec ? n / 4 : 0;
    bool bad = false;
    for (size_t q = i; q < n4; q += stride) {
        f32x4 t = ((f32x4*)x)[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) { bad |= (t[k] != t[k]); t[k] = clamp_keep_nan(t[k], c); }
        ((f32x4*)x)[q] = t;
    }
    for (size_t e = n4 * 4 + i; e < n; e += stride) { bad |= (x[e] != x[e]); x[e] = clamp_keep_nan(x[e], c); }
    if (health && bad) health[1] = 1;
}

}  // namespace

static inline int sp_for(int max_label_len) { return ((2 * max_label_len + 1 + 63) / 64) * 64; }

extern "C" size_t vocr_ctc_workspace_bytes(int t, int b, int v, int max_label_len) {
    if (t <= 0 || b <= 0 || v <= 0 || max_label_len < 0) return 0;
    const size_t sp = sp_for(max_label_len);
    return ((size_t)t * b * v + (size_t)b * 2 * t * sp) * sizeof(float);
}

extern "C" int vocr_ctc_loss_grad(const float* logits, const int32_t* labels, const int32_t* label_offsets,
                                  const int32_t* label_lens, const int32_t* act_lens, float* nll, float* dlogits,
                                  void* workspace, int t, int b, int v, int max_label_len, void* stream) {
    VOCR_CHECK_ARG(logits && labels && label_offsets && label_lens && act_lens && nll && workspace, "vocr_ctc_loss_grad: null pointer");
    VOCR_CHECK_ARG(t > 0 && b > 0 && v > 1 && max_label_len >= 0, "vocr_ctc_loss_grad: bad shape");
    const int sp = sp_for(max_label_len);
    VOCR_CHECK_ARG((size_t)(2 * (sp + 4) + sp) * 4 <= 64 * 1024 && (size_t)4 * v * 4 <= 64 * 1024,
                   "vocr_ctc_loss_grad: label length %d or alphabet %d too large", max_label_len, v);
    hipStream_t s = (hipStream_t)stream;
    float* lp = (float*)workspace;
    float* ab = lp + (size_t)t * b * v;
    const int rows = t * b;
    log_softmax_rows_kernel<<<vocr_cdiv(rows, 4), 256, 0, s>>>(logits, lp, rows, v);
    VOCR_CHECK_LAUNCH("vocr_ctc_loss_grad(log_softmax)");
    const size_t smem = (size_t)(2 * (sp + 4) + sp) * sizeof(float);
    if (sp == 64) ctc_alpha_beta_reg_kernel<1><<<2 * b, 64, 0, s>>>(lp, labels, label_offsets, label_lens, act_lens, ab, nll, t, b, v);
    else if (sp == 128) ctc_alpha_beta_reg_kernel<2><<<2 * b, 64, 0, s>>>(lp, labels, label_offsets, label_lens, act_lens, ab, nll, t, b, v);
    else ctc_alpha_beta_lds_kernel<<<2 * b, 64, smem, s>>>(lp, labels, label_offsets, label_lens, act_lens, ab, nll, t, b, v, sp);
    VOCR_CHECK_LAUNCH("vocr_ctc_loss_grad(alpha_beta)");
    if (dlogits) {
        ctc_grad_kernel<<<vocr_cdiv(rows, 4), 256, (size_t)4 * v * sizeof(float), s>>>(lp, labels, label_offsets, label_lens,
                                                                                      act_lens, ab, nll, dlogits, t, b, v, sp);
        VOCR_CHECK_LAUNCH("vocr_ctc_loss_grad(grad)");
    }
    return VOCR_OK;
}

extern "C" int vocr_argmax_rows(const float* x, int32_t* idx, float* maxv, int rows, int v, void* stream) {
    VOCR_CHECK_ARG(x && idx && maxv && rows > 0 && v > 0, "vocr_argmax_rows: bad argument");
    argmax_rows_kernel<<<vocr_cdiv(rows, 4), 256, 0, (hipStream_t)stream>>>(x, idx, maxv, rows, v);
    VOCR_CHECK_LAUNCH("vocr_argmax_rows");
    return VOCR_OK;
}

extern "C" int vocr_greedy_collapse(const int32_t* idx, const float* maxv, const int32_t* lens, const int32_t* canon,
                                    int32_t* out_labels, int32_t* out_counts, int t, int b, float thresh, void* stream) {
    VOCR_CHECK_ARG(idx && maxv && lens && canon && out_labels && out_counts && t > 0 && b > 0, "vocr_greedy_collapse: bad argument");
    greedy_collapse_kernel<<<vocr_cdiv(b, 64), 64, 0, (hipStream_t)stream>>>(idx, maxv, lens, canon, out_labels, out_counts, t, b, thresh);
    VOCR_CHECK_LAUNCH("vocr_greedy_collapse");
    return VOCR_OK;
}

extern "C" int vocr_clamp_adam(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1,
                               float beta2, float eps, float weight_decay, float clamp, float grad_scale, int step,
                               int32_t* health, void* stream) {
    VOCR_CHECK_ARG(p && g && m && v && step >= 1, "vocr_clamp_adam: bad argument");
    VOCR_CHECK_ARG(clamp >= 0.f, "vocr_clamp_adam: clamp must be >= 0 (got %g)", (double)clamp);   // false for NaN too, as in vocr_clamp
    if (count == 0) return VOCR_OK;
    // bias corrections in double on the host, exactly the scalars torch.optim.Adam derives per step
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
    size_t gsz = (count + 255) / 256;
    if (gsz > 4096) gsz = 4096;
    clamp_adam_kernel<<<(int)gsz, 256, 0, (hipStream_t)stream>>>(p, g, m, v, count, lr, omb1, beta2, omb2, eps, weight_decay, clamp,
                                                                grad_scale, step_size, bc2_sqrt, health);
    VOCR_CHECK_LAUNCH("vocr_clamp_adam");
    return VOCR_OK;
}

extern "C" int vocr_clamp(float* x, size_t count, float clamp, int32_t* health, void* stream) {
    VOCR_CHECK_ARG(x && clamp >= 0.f, "vocr_clamp: bad argument");
    if (count == 0) return VOCR_OK;
    size_t gsz = (count / 4 + 255) / 256;
    if (gsz > 2048) gsz = 2048;
    if (gsz < 1) gsz = 1;
    clamp_kernel<<<(int)gsz, 256, 0, (hipStream_t)stream>>>(x, count, clamp, ((((uintptr_t)x) & 15) == 0) ? 1 : 0, health);
    VOCR_CHECK_LAUNCH("vocr_clamp");
    return VOCR_OK;
}
