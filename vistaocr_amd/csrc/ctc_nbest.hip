// Weighted n-best CTC scores and gradient: for n labellings of the same line, out_ctc[b][q] = ln P_ctc(labels[b][q] | x_b) and
//   dlogits = d/dlogits sum_b sum_q weights[b][q] * ln P_ctc(labels[b][q] | x_b)
// in ONE [T][B][V] tensor - what an expected-error (minimum-error-rate) criterion over a beam search's n-best list needs, where the
// composition of vocr_ctc_loss_grad calls needs n copies of the logits, n log-softmaxes, n gradient tensors and a reduction, and has
// no classes.  Inputs and conventions are vocr_ctc_align's: blank = 0, S = 2L+1 extended positions, the skip s-2 -> s iff position s is
// not blank and its CLASS differs from that of s-2, classes from canon[V].
//
// With p_t(v) the softmax of frame t, P_t(c) the sum of p_t over the columns of class c, alpha_t(s) / beta_t(s) the forward / backward
// lattices of labelling q (beta includes the emission at t) and P_q its probability,
//   occ_q(t, c) = sum over the positions s of class c of alpha_t(s) * beta_t(s) / (P_t(c) * P_q)         (sums to 1 over c)
//   dlogits[t][b][v] = p_t(v) / P_t(class(v)) * sum_q w_q occ_q(t, class(v))  -  p_t(v) * sum_q w_q
// the sums over the hypotheses with a finite score.
//
//   kernel 1  class log-probabilities : class_logprob_rows_kernel of the alignment, once per line.
//   kernel 2  lattices (ctc_lattice.h): ctc_lattice_kernel over SumCell (ctc_label_sweep's plain sum), as the edit scores.  With
//                                       weights: one wave per (line, hypothesis, direction) writes alpha or beta TRANSPOSED ([s][t])
//                                       to the workspace and the forward wave out_ctc.  Without: the forward wave alone, nothing
//                                       stored.  out_ctc holds the bits of vocr_ctc_edit_scores's either way.
//   kernel 3  gradient                : one wave per (line, tile of TT frames).  Lane (g, k) owns frame k of the tile for the
//                                       hypotheses q = g, g + NG, ..: it walks their positions s in order and adds
//                                       w_q * exp(alpha + beta - ln P_t(c) - ln P_q) to ITS OWN accumulator of class c in LDS
//                                       (acc[g][c][k]: consecutive lanes, consecutive banks), reading alpha and beta along t
//                                       (coalesced, TT * 4 bytes per position).  No two lanes share an accumulator, so there is no
//                                       reduction inside the loop, no atomic, and the order of every sum is fixed.  Then
//                                       ctc_grad_rows (ctc_lattice.h), the row pass shared with the entropy's gradient: frame by
//                                       frame the row's log-softmax again, the NG partial sums added in order, one coalesced store of
//                                       the row.  Rows t >= lens[b] are written as zeros.
// A term with alpha or beta at -inf is skipped and a column with p_t(v) = 0 gets share 0, so a class with P_t(c) = 0 never meets a
// division; a hypothesis with a -inf score is skipped whole, whatever its weight.  A line's rows are computed from that line alone.
#include "ctc_lattice.h"

namespace {

// grid.x = B * ceil(T / TT) (tile fastest), 64 threads.  Dynamic LDS: acc[NG][V][TT] floats.
__global__ __launch_bounds__(64) void ctc_nbest_grad_kernel(const float* __restrict__ logits, const float* __restrict__ clp,
                                                            const int32_t* __restrict__ lens, const int32_t* __restrict__ canon,
                                                            const int32_t* __restrict__ labels, const int32_t* __restrict__ label_lens,
                                                            int T, int B, int V, int n, int label_stride, int max_label_len,
                                                            const float* __restrict__ lat, const float* __restrict__ scores,
                                                            const float* __restrict__ weights, float* __restrict__ dlogits) {
    extern __shared__ __attribute__((aligned(16))) float acc[];
    const int lane = threadIdx.x, k = lane & (TT - 1), g = lane / TT;
    const int tiles = (T + TT - 1) / TT;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT, t = t0 + k;
    const int len = min(max(lens[b], 0), T);
    const long tstride = (long)B * V;
    for (int i = lane; i < NG * V * TT; i += 64) acc[i] = 0.f;
    __syncthreads();
    const bool live = t < len;
    const float* lpt = clp + (long)(live ? t : 0) * tstride + (long)b * V;      // the frame's class log-probabilities
    const long SM = 2 * (long)max_label_len + 1;
    float* mine = acc + (long)g * V * TT + k;                                   // mine[c * TT]
    float wsum = 0.f;                                                            // of this lane's hypotheses; the same for every k
    for (int q = g; q < n; q += NG) {
        const int prob = b * n + q;
        const float sc = scores[prob];
        if (!(sc > NEG_INF)) continue;                                           // no path: contributes nothing
        const float w = weights[prob];
        wsum += w;
        if (!live) continue;
        const int S = 2 * label_lens[prob] + 1;
        const int32_t* lab = labels + (long)prob * label_stride;
        const float* alpha = lat + (long)prob * 2 * SM * T + t;
        const float* beta = alpha + SM * T;
#pragma unroll 4
        for (int s = 0; s < S; ++s) {
            const int e = (s & 1) ? lab[s >> 1] : 0;
            const float a = alpha[(long)s * T], be = beta[(long)s * T];
            if (a == NEG_INF || be == NEG_INF) continue;
            const float lp = lpt[e];                                             // finite: alpha is
            mine[class_of(canon, e) * TT] += w * expf(a + be - lp - sc);
        }
    }
    float wtot = __shfl(wsum, 0, 64);
#pragma unroll
    for (int j = 1; j < NG; ++j) wtot += __shfl(wsum, j * TT, 64);
    __syncthreads();
    ctc_grad_rows(logits, clp, canon, acc, T, B, V, b, t0, len, wtot, dlogits, lane);
}

}  // namespace

extern "C" size_t vocr_ctc_nbest_workspace_bytes(int t, int b, int v, int n, int max_label_len) {
    const LatticePlan p = lattice_plan(t, b, v, n, max_label_len, SumCell::ROWS);
    if (!p.ok) return 0;
    return clp_bytes(t, b, v) + p.lattice_bytes;
}

extern "C" int vocr_ctc_nbest_grad(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                   const int32_t* labels, const int32_t* label_lens, int n, int label_stride, int max_label_len,
                                   const float* weights, float* out_ctc, float* dlogits, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const char* who = "vocr_ctc_nbest_grad";
    VOCR_CHECK_ARG(logits && lens && labels && label_lens && out_ctc && workspace, "%s: null pointer", who);
    VOCR_CHECK_ARG(!weights == !dlogits, "vocr_ctc_nbest_grad: weights and dlogits go together (weights %s, dlogits %s)",
                   weights ? "given" : "NULL", dlogits ? "given" : "NULL");
    if (check_labelling_shape(who, t, b, v, n, label_stride, max_label_len) != VOCR_OK) return VOCR_EINVAL;
    const LatticePlan p = lattice_plan(t, b, v, n, max_label_len, SumCell::ROWS);
    VOCR_CHECK_ARG(p.ok, "vocr_ctc_nbest_grad: unsupported shape (t=%d b=%d v=%d n=%d max_label_len=%d): the lattices of all "
                   "labellings (%zu bytes) must fit %zu bytes and one row of the sweep (%zu bytes) the LDS", t, b, v, n, max_label_len,
                   p.lattice_bytes, LATTICE_BYTES_MAX, p.lds);
    // a scores-only call stores no lattice and needs the class log-probabilities alone
    const size_t need = clp_bytes(t, b, v) + (weights ? p.lattice_bytes : 0);
    VOCR_CHECK_ARG(workspace_bytes >= need, "vocr_ctc_nbest_grad: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_lattice_kernel<SumCell, true>, (const void*)ctc_lattice_kernel<SumCell, false>,
                               (const void*)ctc_nbest_grad_kernel};
    if (vocr_allow_dynamic_lds(big, 3, (int)LDS_BUDGET, &lds_set, who) != VOCR_OK) return VOCR_ELAUNCH;
    float* clp = (float*)workspace;
    float* lat = (float*)((char*)workspace + clp_bytes(t, b, v));
    if (launch_class_logprob(who, logits, lens, canon, clp, t, b, v, s) != VOCR_OK) return VOCR_ELAUNCH;
    if (!weights) {
        ctc_lattice_kernel<SumCell, false><<<b * n, 64, p.lds, s>>>(clp, lens, canon, labels, label_lens, t, b, v, n, label_stride,
                                                                    max_label_len, p.sp, nullptr, out_ctc, nullptr);
        VOCR_CHECK_LAUNCH("vocr_ctc_nbest_grad(scores)");
        return VOCR_OK;
    }
    ctc_lattice_kernel<SumCell, true><<<b * n * 2, 64, p.lds, s>>>(clp, lens, canon, labels, label_lens, t, b, v, n, label_stride,
                                                                   max_label_len, p.sp, lat, out_ctc, nullptr);
    VOCR_CHECK_LAUNCH("vocr_ctc_nbest_grad(lattices)");
    ctc_nbest_grad_kernel<<<b * vocr_cdiv(t, TT), 64, (size_t)NG * v * TT * sizeof(float), s>>>(
        logits, clp, lens, canon, labels, label_lens, t, b, v, n, label_stride, max_label_len, lat, out_ctc, weights, dlogits);
    VOCR_CHECK_LAUNCH("vocr_ctc_nbest_grad(gradient)");
    return VOCR_OK;
}
