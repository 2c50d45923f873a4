// CTC edit scores: the exact CTC forward score ln P_ctc(labelling' | x) of EVERY labelling one edit away from a hypothesis - each
// substitution of one label by another class, each deletion, each insertion of a class between two labels.  What a per-character
// posterior, ranked alternatives and a "something is missing here" signal are made of (the reference got them from eesen's lattice and
// the confidence experiment of src/conf_test.py).  Inputs and conventions are vocr_ctc_align's: blank = 0, extended sequence of
// S = 2L+1 positions, the skip s-2 -> s iff position s is not blank and its CLASS differs from that of s-2, classes from canon[V].
//
// alpha[t][s] / beta[t][s] are the forward / backward lattices of the hypothesis (beta includes the emission at t).  alpha up to
// position 2p and beta from position 2p+2 do not depend on label p, so an edit at p is a recursion over one or two NEW states between
// them, x (the edited or inserted label) and y (the blank behind an inserted label):
//   x(0) = lp(0,c) if p = 0 else -inf;   x(t) = lp(t,c) + lse(x(t-1), alpha[t-1][2p], alpha[t-1][2p-1] if p > 0 and c != l(p-1))
//   y(0) = -inf;                         y(t) = lp(t,0) + lse(y(t-1), x(t-1))
//   substitution p -> c : lse_t x(t) + e(t),  e(t) = lse(beta[t+1][2p+2], beta[t+1][2p+3] if p < L-1 and c != l(p+1)),
//                         e(len-1) = 0 if p = L-1 else -inf
//   deletion of p       : p = 0: lse(beta[0][2], beta[0][3] if L > 1);  else lse_t alpha[t][2p-1] + e(t), the skip iff l(p-1) != l(p+1)
//   insertion of c at q : q < L: lse_t<len-1 of (x(t) + beta[t+1][2q+1] if c != l(q)) and y(t) + beta[t+1][2q+1];  q = L: x(len-1), y(len-1)
// ("!=" compares classes).  Every sum cuts a path at its last frame in a given state, so no path is counted twice.
//
//   kernel 1  class log-probabilities : class_logprob_rows_kernel of the alignment, once per line.
//   kernel 2  lattices (ctc_lattice.h): ctc_lattice_kernel<SumCell, true>: one wave per (line, hypothesis, direction) writes alpha or
//                                       beta to the workspace, TRANSPOSED ([s][t]: kernel 3 walks one position through the frames), by
//                                       ctc_label_sweep over SumCell, the plain sum, which the n-best gradient runs too (the alignment
//                                       entropy runs it over its own cell).  beta is alpha of the reversed labelling over the reversed
//                                       frames, so both directions run the same code.  The forward wave also writes ln P_ctc(labels | x).
//   kernel 3  edit scores             : one workgroup per (line, hypothesis, slot p), p = 0 .. max_label_len; thread c owns column c
//                                       (coalesced class log-probabilities).  One pass over the frames serves the substitution at p,
//                                       the insertion before p (the same x) and the deletion of p.  The alpha / beta values of a
//                                       frame are the same for the whole workgroup and, like the column's own log-probability,
//                                       are loaded PF frames ahead.  The sums over t are kept as (max, sum): one exponential per
//                                       term and one logarithm at the end.  No LDS, no barrier.
// Every float is computed by a fixed thread in a fixed order and the only cross-lane operations are shuffles and ballots: results are
// bit-identical from run to run, and columns of one class (which read the same class log-probabilities) hold the same bits.
#include "ctc_lattice.h"

namespace {

// what kernel 3 needs of one frame t: the column's and the blank's class log-probability, alpha[t][2p], alpha[t][2p-1] and
// beta[t+1][2p+1 .. 2p+3] (-inf where the position does not exist)
struct EditFrame {
    float lpc, lp0, a0, a1, b1, b2, b3;
};

// grid.x = B * n * (max_label_len + 1), V rounded up to 64 threads.
__global__ __launch_bounds__(256) void ctc_edit_scores_kernel(const float* __restrict__ clp, const int32_t* __restrict__ lens,
                                                              const int32_t* __restrict__ canon, const int32_t* __restrict__ labels,
                                                              const int32_t* __restrict__ label_lens, int T, int B, int V, int n,
                                                              int label_stride, int max_label_len, const float* __restrict__ lat,
                                                              float* __restrict__ out_sub, float* __restrict__ out_del,
                                                              float* __restrict__ out_ins) {
    const int M = max_label_len;
    const int prob = blockIdx.x / (M + 1), p = blockIdx.x - prob * (M + 1), b = prob / n;
    const int c = threadIdx.x, cc = min(c, V - 1);
    const int len = min(max(lens[b], 0), T);
    const int L = label_lens[prob];
    const int32_t* lab = labels + (long)prob * label_stride;
    float* sub = p < M ? out_sub + ((long)prob * M + p) * V : nullptr;
    float* del = p < M ? out_del + (long)prob * M + p : nullptr;
    float* ins = out_ins + ((long)prob * (M + 1) + p) * V;
    const bool bad = labelling_bad(canon, lab, L, V, M, threadIdx.x & 63);
    if (bad || p > L || len == 0) {
        if (c < V) {
            ins[c] = NEG_INF;
            if (sub) sub[c] = NEG_INF;
        }
        // no frames: the one labelling with a score is the empty one, which the deletion of an only label leaves
        if (c == 0 && del) *del = (!bad && len == 0 && L == 1 && p == 0) ? 0.f : NEG_INF;
        return;
    }
    const int cls_c = class_of(canon, cc);
    const int cls_m1 = p > 0 ? class_of(canon, lab[p - 1]) : -1;
    const int cls_0 = p < L ? class_of(canon, lab[p]) : -1;
    const int cls_p1 = p < L - 1 ? class_of(canon, lab[p + 1]) : -1;
    const bool skip_a = p > 0 && cls_c != cls_m1;                // x may be entered from label p-1
    const bool skip_b = p < L - 1 && cls_c != cls_p1;            // a substituted x may leave to label p+1
    const bool ins_x = p < L && cls_c != cls_0;                  // an inserted x may leave to label p
    const bool skip_d = p > 0 && p < L - 1 && cls_m1 != cls_p1;  // label p-1 may leave to label p+1 once p is deleted
    const long tstride = (long)B * V;
    const float* lpb = clp + (long)b * V;
    const long SM = 2 * (long)M + 1;
    const float* alpha = lat + (long)prob * 2 * SM * T;
    const float* beta = alpha + SM * T;
    const float* A0 = alpha + (long)(2 * p) * T;
    const float* A1 = p > 0 ? alpha + (long)(2 * p - 1) * T : nullptr;
    const float* B1 = p < L ? beta + (long)(2 * p + 1) * T : nullptr;
    const float* B2 = p < L ? beta + (long)(2 * p + 2) * T : nullptr;
    const float* B3 = p < L - 1 ? beta + (long)(2 * p + 3) * T : nullptr;

    auto load = [&](int t) {
        EditFrame f;
        t = min(t, len - 1);
        const int tb = min(t + 1, len - 1);
        f.lpc = lpb[t * tstride + cc];
        f.lp0 = lpb[t * tstride];
        f.a0 = A0[t];
        f.a1 = A1 ? A1[t] : NEG_INF;
        f.b1 = B1 ? B1[tb] : NEG_INF;
        f.b2 = B2 ? B2[tb] : NEG_INF;
        f.b3 = B3 ? B3[tb] : NEG_INF;
        return f;
    };

    LseAcc acc_sub, acc_ins, acc_del;
    if (p == 0 && L > 0) acc_del.add(lse2(B2[0], B3 ? B3[0] : NEG_INF));
    const float e_last = p == L - 1 ? 0.f : NEG_INF;
    float x = NEG_INF, y = NEG_INF, pa0 = NEG_INF, pa1 = NEG_INF;
    EditFrame buf[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) buf[k] = load(k);
    for (int t0 = 0; t0 < len; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            if (t < len) {                                       // uniform
                const EditFrame f = buf[k];
                buf[k] = load(t + PF);
                const float xn = (t == 0 ? (p == 0 ? 0.f : NEG_INF) : lse3(x, pa0, skip_a ? pa1 : NEG_INF)) + f.lpc;
                const float yn = t == 0 ? NEG_INF : lse2(y, x) + f.lp0;
                const bool last = t == len - 1;
                if (p < L) {
                    const float e23 = last ? e_last : lse2(f.b2, f.b3);
                    const float e2 = last ? e_last : f.b2;
                    acc_sub.add(xn + (skip_b ? e23 : e2));
                    if (!last) {
                        if (ins_x) acc_ins.add(xn + f.b1);
                        acc_ins.add(yn + f.b1);
                    }
                    if (p > 0) acc_del.add(f.a1 + (skip_d ? e23 : e2));
                } else if (last) {
                    acc_ins.add(xn);
                    acc_ins.add(yn);
                }
                x = xn;
                y = yn;
                pa0 = f.a0;
                pa1 = f.a1;
            }
        }
    }
    if (c < V) {
        const bool valid = c > 0 && cls_c != 0;                  // the blank's class is no edit
        ins[c] = valid ? acc_ins.get() : NEG_INF;
        if (sub) sub[c] = (valid && p < L) ? acc_sub.get() : NEG_INF;
    }
    if (c == 0 && del) *del = p < L ? acc_del.get() : NEG_INF;
}

// kernel 3's grid, B * n * (max_label_len + 1) workgroups, is this entry's own limit
LatticePlan edit_plan(int t, int b, int v, int n, int max_label_len) {
    if ((long)b * n * (max_label_len + 1) >= (1L << 31)) return LatticePlan{0, 0, 0, false};
    return lattice_plan(t, b, v, n, max_label_len, SumCell::ROWS);
}

}  // namespace

extern "C" size_t vocr_ctc_edit_workspace_bytes(int t, int b, int v, int n, int max_label_len) {
    const LatticePlan p = edit_plan(t, b, v, n, max_label_len);
    if (!p.ok) return 0;
    return clp_bytes(t, b, v) + p.lattice_bytes;
}

extern "C" int vocr_ctc_edit_scores(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                    const int32_t* labels, const int32_t* label_lens, int n, int label_stride, int max_label_len,
                                    float* out_ctc, float* out_sub, float* out_del, float* out_ins, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "vocr_ctc_edit_scores";
    VOCR_CHECK_ARG(logits && lens && labels && label_lens && out_ctc && out_sub && out_del && out_ins && workspace, "%s: null pointer", who);
    if (check_labelling_shape(who, t, b, v, n, label_stride, max_label_len) != VOCR_OK) return VOCR_EINVAL;
    const LatticePlan p = edit_plan(t, b, v, n, max_label_len);
    VOCR_CHECK_ARG(p.ok, "vocr_ctc_edit_scores: unsupported shape (t=%d b=%d v=%d n=%d max_label_len=%d): the lattices of all labellings "
                   "(%zu bytes) must fit %zu bytes and one row of the sweep (%zu bytes) the LDS", t, b, v, n, max_label_len,
                   p.lattice_bytes, LATTICE_BYTES_MAX, p.lds);
    const size_t need = vocr_ctc_edit_workspace_bytes(t, b, v, n, max_label_len);
    VOCR_CHECK_ARG(workspace_bytes >= need, "vocr_ctc_edit_scores: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_lattice_kernel<SumCell, true>};
    if (vocr_allow_dynamic_lds(big, 1, (int)LDS_BUDGET, &lds_set, who) != VOCR_OK) return VOCR_ELAUNCH;
    float* clp = (float*)workspace;
    float* lat = (float*)((char*)workspace + clp_bytes(t, b, v));
    if (launch_class_logprob(who, logits, lens, canon, clp, t, b, v, s) != VOCR_OK) return VOCR_ELAUNCH;
    ctc_lattice_kernel<SumCell, true><<<b * n * 2, 64, p.lds, s>>>(clp, lens, canon, labels, label_lens, t, b, v, n, label_stride,
                                                                   max_label_len, p.sp, lat, out_ctc, nullptr);
    VOCR_CHECK_LAUNCH("vocr_ctc_edit_scores(lattices)");
    ctc_edit_scores_kernel<<<b * n * (max_label_len + 1), vocr_cdiv(v, 64) * 64, 0, s>>>(clp, lens, canon, labels, label_lens, t, b, v, n,
                                                                                        label_stride, max_label_len, lat, out_sub,
                                                                                        out_del, out_ins);
    VOCR_CHECK_LAUNCH("vocr_ctc_edit_scores(scores)");
    return VOCR_OK;
}
