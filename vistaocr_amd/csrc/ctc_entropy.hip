// Alignment entropy of a labelling and its gradient (entropy-regularised CTC, Liu, Jin and Zhang 2018): for the labelling l of line b,
//   out_ctc[b] = ln P,  P = sum over the frame paths pi with B(pi) = l of p(pi),            p(pi) = prod_t P_t(pi_t)
//   out_entropy[b] = H = - sum_pi (p / P) ln (p / P) = N / P + ln P,                         N = sum_pi p(pi) * (-ln p(pi))
// and, with coeff[b] = (w_ctc, w_ent) given, dlogits = d/dlogits sum_b (w_ctc * ln P_b + w_ent * H_b) in one [T][B][V] tensor.  Inputs and
// conventions are vocr_ctc_nbest_grad's with n = 1: blank = 0, S = 2L+1 extended positions, the skip s-2 -> s iff position s is not
// blank and its CLASS differs from that of s-2, classes from canon[V], u_t(c) = ln P_t(c) from class_logprob_rows_kernel.
//
// H needs a second quantity beside the path sum (an expectation semiring).  WHICH ONE: not h = ln sum p * (-ln p).  That pair was
// built and measured first: a and h are both about ln P (-1000 on dense logits at T = 294), each good to about 1e-3 after 294 steps,
// and N / P = exp(h - a) is about |ln P| with that RELATIVE error, so H = N / P + ln P was off by 0.4 to 1 nat and its gradient by
// the size of the gradient.  The pair here is (a, e), e_t(s) = the ENTROPY of the posterior over the partial paths that end in (t, s):
//   w_i = exp(a_i - A) over the allowed predecessors i,  A = lse3 of a_(t-1)(i)          (the terms lse3 forms anyway)
//   a_t(s) = A + u                                            the expression of ctc_label_sweep: out_ctc holds vocr_ctc_nbest_grad's bits
//   e_t(s) = sum_i w_i * (e_(t-1)(i) - ln w_i)                the entropy of a mixture of disjoint path sets; e = 0 at t = 0
//   H = the same sum over the two end states with w = exp(a_end - ln P).
// The frame's own factor u multiplies every path through (t, s) alike and leaves e alone, so e is a convex combination of numbers of
// the size of H plus a term in [0, ln 3]: linear domain, every term >= 0, nothing of the size of ln P in it.  -ln w_i is taken as
// (m - a_i) + ln(sum), m the maximum, not as A - a_i.  A line with one feasible path has e = 0 in every cell and H = 0 exactly.
//
//   kernel 1  class log-probabilities : class_logprob_rows_kernel, once per line.
//   kernel 2  lattices (ctc_lattice.h): ctc_lattice_kernel with n = 1 over EntCell below, the (a, e) cell: ctc_label_sweep, the sweep
//                                       of the edit scores and the n-best gradient in both of its row layouts, with the e row beside
//                                       the a row.  With coeff: one wave per (line, direction) writes its pair TRANSPOSED ([s][t]) to
//                                       the workspace - the backward pair is the forward pair of the reversed labelling over the
//                                       reversed frames: b includes frame t's emission, eb is the entropy over the partial paths that
//                                       START in (t, s) - and the forward wave out_ctc and out_entropy.  Without: the forward wave alone.
//   kernel 3  gradient                : one wave per (line, tile of TT frames).  Lane (g, k) owns frame k of the tile for the positions
//                                       s = g, g + NG, ..: it adds its term to ITS OWN accumulator of the position's class in LDS
//                                       (acc[g][c][k]), so there is no atomic and every sum has a fixed order; then ctc_grad_rows, the
//                                       row pass the n-best gradient ends with (log-softmax again, the NG partial sums in order, one
//                                       coalesced store).
//
// The gradient.  gam(t, s) = exp(a + b - u - ln P) is the posterior of position s at frame t and occ(t, c) its sum over the positions of
// class c, as in vocr_ctc_nbest_grad.  With occN(t, c) = (1 / P) sum over the paths with pi_t = c of p * (-ln p):
//   dH/du_t(c) = occN - (N / P) occ = sum over the positions s of class c of gam * (ef + eb - ln gam - H)
// (the paths through (t, s) are a prefix times a suffix, so their entropy is ef + eb, and H = sum_s gam * (ef + eb - ln gam) at every
// frame: the derivative sums to 0 over c and the log-softmax adds no correction):
//   dlogits[t][v] = share_t(v) * sum_s gam * (w_ctc + w_ent (ef + eb - ln gam - H)) - p_t(v) w_ctc,        share = p_t(v) / P_t(class(v)).
// WHICH COMBINATION: the same-frame one, forward and backward pair both at frame t.  In the (a, h) form that costs a subtraction (frame
// t's -u is in both halves); in this form nothing is counted twice, because u is in no entropy: four reads per cell, one exponential,
// no difference of large numbers except the exponent a + b - u - ln P that the CTC gradient has as well.  The alternative (the forward
// pair at t with the successors' backward pair at t + 1) reads up to three successors' pairs per cell and needs the end states as a
// special case, and buys nothing here.
//
// LIMIT: the S > 64 layout keeps two rows, ext and TB staged frames: sweep_floats(sp, 2) = 2 (sp + 2) + sp + TB sp = 11 sp + 4 floats <=
// LDS_BUDGET / 4 = 36864 gives sp <= 3328 (52 chunks), so max_label_len <= 1663 (2 * 1663 + 1 = 3327), where the single-row scorers
// reach 1823.
#include "ctc_lattice.h"

namespace {

constexpr int ENTROPY_MAX_LABEL_LEN = 1663;    // what lattice_plan's LDS check admits for two rows; named for the error text
static_assert(sweep_floats(3328, 2) * 4 <= LDS_BUDGET && sweep_floats(3392, 2) * 4 > LDS_BUDGET, "ENTROPY_MAX_LABEL_LEN");
static_assert(2 * ENTROPY_MAX_LABEL_LEN + 1 <= 3328 && 2 * (ENTROPY_MAX_LABEL_LEN + 1) + 1 > 3328, "ENTROPY_MAX_LABEL_LEN");

// The mixture of up to three disjoint path sets with log-masses a1..a3 and entropies e1..e3: A = lse3(a1, a2, a3) in lse3's own
// expression (the same terms in the same order, so the same bits) and e = sum w_i (e_i - ln w_i), w_i = exp(a_i - A).  A set at -inf
// has no share; all at -inf: (-inf, 0).
struct Mix {
    float A, e;
};

__device__ __forceinline__ Mix mix3(float a1, float a2, float a3, float e1, float e2, float e3) {
    const float m = fmaxf(a1, fmaxf(a2, a3));
    if (m == NEG_INF) return {NEG_INF, 0.f};
    const float x1 = expf(a1 - m), x2 = expf(a2 - m), x3 = expf(a3 - m);
    const float sum = x1 + x2 + x3;
    const float lg = logf(sum);
    float acc = 0.f;
    if (a1 > NEG_INF) acc += x1 * (e1 + ((m - a1) + lg));
    if (a2 > NEG_INF) acc += x2 * (e2 + ((m - a2) + lg));
    if (a3 > NEG_INF) acc += x3 * (e3 + ((m - a3) + lg));
    return {lg + m, acc / sum};
}

// The cell of ctc_label_sweep that carries the pair.  kill() masks a alone: mix3 gives a set at -inf no share, whatever its e.  A cell
// without a path has e = 0.  finish(): ln P and H, the mixture of the two end cells.
struct EntCell {
    static constexpr int ROWS = 2;
    static constexpr bool ENTROPY = true;
    float a, e;
    static __device__ __forceinline__ EntCell none() { return {NEG_INF, 0.f}; }
    static __device__ __forceinline__ EntCell first(float u) { return {u, 0.f}; }
    static __device__ __forceinline__ EntCell step(EntCell p1, EntCell p2, EntCell p3, float u) {
        const Mix mx = mix3(p1.a, p2.a, p3.a, p1.e, p2.e, p3.e);
        const float a = mx.A + u;
        return {a, a > NEG_INF ? mx.e : 0.f};
    }
    __device__ __forceinline__ void kill() { a = NEG_INF; }
    __device__ __forceinline__ EntCell up(int d) const { return {__shfl_up(a, d, 64), __shfl_up(e, d, 64)}; }
    __device__ __forceinline__ EntCell from(int l) const { return {__shfl(a, l, 64), __shfl(e, l, 64)}; }
    static __device__ __forceinline__ EntCell get(const float* p, long stride, long i) { return {p[i], p[stride + i]}; }
    __device__ __forceinline__ void put(float* p, long stride, long i) const { p[i] = a, p[stride + i] = e; }
    static __device__ __forceinline__ void finish(EntCell as, EntCell cs, float* out_ctc, float* out_entropy, int i) {
        const Mix end = mix3(as.a, cs.a, NEG_INF, as.e, cs.e, 0.f);
        out_ctc[i] = end.A;
        out_entropy[i] = fmaxf(end.e, 0.f);                      // 0 without a path
    }
};

// grid.x = B * ceil(T / TT) (tile fastest), 64 threads.  Dynamic LDS: acc[NG][V][TT] floats.
__global__ __launch_bounds__(64) void ctc_entropy_grad_kernel(const float* __restrict__ logits, const float* __restrict__ clp,
                                                              const int32_t* __restrict__ lens, const int32_t* __restrict__ canon,
                                                              const int32_t* __restrict__ labels, const int32_t* __restrict__ label_lens,
                                                              int T, int B, int V, int label_stride, int max_label_len,
                                                              const float* __restrict__ lat, const float* __restrict__ scores,
                                                              const float* __restrict__ entropy, const float* __restrict__ coeff,
                                                              float* __restrict__ dlogits) {
    extern __shared__ __attribute__((aligned(16))) float acc[];
    const int lane = threadIdx.x, k = lane & (TT - 1), g = lane / TT;
    const int tiles = (T + TT - 1) / TT;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT, t = t0 + k;
    const int len = min(max(lens[b], 0), T);
    const long tstride = (long)B * V;
    const float sc = scores[b];
    const bool scored = sc > NEG_INF;                            // no path: the line's rows are zeros
    const float wc = coeff[2 * b], we = coeff[2 * b + 1];
    for (int i = lane; i < NG * V * TT; i += 64) acc[i] = 0.f;
    __syncthreads();
    if (scored && t < len) {
        const float* lpt = clp + (long)t * tstride + (long)b * V;               // the frame's class log-probabilities
        const long SM = 2 * (long)max_label_len + 1;
        const float H = entropy[b];
        const int S = 2 * label_lens[b] + 1;
        const int32_t* lab = labels + (long)b * label_stride;
        const float* fa = lat + (long)b * 4 * SM * T + t;                       // a, ef, b, eb: planes of SM * T
        float* mine = acc + (long)g * V * TT + k;                               // mine[c * TT]
#pragma unroll 2
        for (int s = g; s < S; s += NG) {
            const float a = fa[(long)s * T], be = fa[(2 * SM + s) * T];
            if (a == NEG_INF || be == NEG_INF) continue;
            const int e = (s & 1) ? lab[s >> 1] : 0;
            const float u = lpt[e];                                             // finite: a is
            const float ef = fa[(SM + s) * T], eb = fa[(3 * SM + s) * T];
            const float lg = a + be - u - sc;                                   // ln gam
            mine[class_of(canon, e) * TT] += expf(lg) * (wc + we * (ef + eb - lg - H));
        }
    }
    __syncthreads();
    ctc_grad_rows(logits, clp, canon, acc, T, B, V, b, t0, scored ? len : 0, wc, dlogits, lane);
}

}  // namespace

extern "C" size_t vocr_ctc_entropy_workspace_bytes(int t, int b, int v, int max_label_len, int want_grad) {
    const LatticePlan p = lattice_plan(t, b, v, 1, max_label_len, EntCell::ROWS);
    if (!p.ok) return 0;
    return clp_bytes(t, b, v) + (want_grad ? p.lattice_bytes : 0);
}

extern "C" int vocr_ctc_entropy(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                const int32_t* labels, const int32_t* label_lens, int label_stride, int max_label_len,
                                const float* coeff, float* out_ctc, float* out_entropy, float* dlogits, void* workspace,
                                size_t workspace_bytes, void* stream) {
    const char* who = "vocr_ctc_entropy";
    VOCR_CHECK_ARG(logits && lens && labels && label_lens && out_ctc && out_entropy && workspace, "%s: null pointer", who);
    VOCR_CHECK_ARG(!coeff == !dlogits, "vocr_ctc_entropy: coeff and dlogits go together (coeff %s, dlogits %s)", coeff ? "given" : "NULL",
                   dlogits ? "given" : "NULL");
    if (check_labelling_shape(who, t, b, v, 1, label_stride, max_label_len) != VOCR_OK) return VOCR_EINVAL;
    const LatticePlan p = lattice_plan(t, b, v, 1, max_label_len, EntCell::ROWS);
    VOCR_CHECK_ARG(p.ok, "vocr_ctc_entropy: unsupported shape (t=%d b=%d v=%d max_label_len=%d): need max_label_len <= %d (the paired rows "
                   "of the sweep in the LDS) and the four lattices (%zu bytes) within %zu bytes", t, b, v, max_label_len,
                   ENTROPY_MAX_LABEL_LEN, p.lattice_bytes, LATTICE_BYTES_MAX);
    // a scores-only call stores no lattice and needs the class log-probabilities alone
    const size_t need = clp_bytes(t, b, v) + (coeff ? p.lattice_bytes : 0);
    VOCR_CHECK_ARG(workspace_bytes >= need, "vocr_ctc_entropy: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_lattice_kernel<EntCell, true>, (const void*)ctc_lattice_kernel<EntCell, false>,
                               (const void*)ctc_entropy_grad_kernel};
    if (vocr_allow_dynamic_lds(big, 3, (int)LDS_BUDGET, &lds_set, who) != VOCR_OK) return VOCR_ELAUNCH;
    float* clp = (float*)workspace;
    float* lat = (float*)((char*)workspace + clp_bytes(t, b, v));
    if (launch_class_logprob(who, logits, lens, canon, clp, t, b, v, s) != VOCR_OK) return VOCR_ELAUNCH;
    if (!coeff) {
        ctc_lattice_kernel<EntCell, false><<<b, 64, p.lds, s>>>(clp, lens, canon, labels, label_lens, t, b, v, 1, label_stride,
                                                               max_label_len, p.sp, nullptr, out_ctc, out_entropy);
        VOCR_CHECK_LAUNCH("vocr_ctc_entropy(scores)");
        return VOCR_OK;
    }
    ctc_lattice_kernel<EntCell, true><<<b * 2, 64, p.lds, s>>>(clp, lens, canon, labels, label_lens, t, b, v, 1, label_stride,
                                                              max_label_len, p.sp, lat, out_ctc, out_entropy);
    VOCR_CHECK_LAUNCH("vocr_ctc_entropy(lattices)");
    ctc_entropy_grad_kernel<<<b * vocr_cdiv(t, TT), 64, (size_t)NG * v * TT * sizeof(float), s>>>(
        logits, clp, lens, canon, labels, label_lens, t, b, v, label_stride, max_label_len, lat, out_ctc, out_entropy, coeff, dlogits);
    VOCR_CHECK_LAUNCH("vocr_ctc_entropy(gradient)");
    return VOCR_OK;
}
