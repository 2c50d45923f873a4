// CTC forced alignment: the best (Viterbi) CTC path of a KNOWN labelling through the frames of a line, the frame span of every label
// on it, per-label scores, and the forward score ln P_ctc(labels | x) from the same sweep.  Stands in for the piece the reference's
// confidence experiment needs and never shipped: conf_utils.form_confidence_gt(model_output, lens, target, target_widths) of
// src/conf_test.py, and the per-frame confidences decode_with_lm_with_conf consumes.
//
// Blank = 0, extended sequence ext[0..S), S = 2L+1 (ext[2p+1] = label p, even positions blank), the transition rule of
// vocr_ctc_loss_grad: s -> s and s-1 -> s always, s-2 -> s iff ext[s] is not blank and its CLASS differs from ext[s-2]'s.  Classes
// are those of vocr_ctc_beam_search: canon[V] sanitised the same way, a class's frame log-probability is the logsumexp of its member
// columns, and a label given as any member index stands for its class.
//
//   kernel 1  class log-probabilities     : one wave per (t, b) row with t < lens[b]: row log-softmax in fp32, then for EVERY column
//                                           the log-probability of its class, clp[t][b][v] (so the sweep gathers by the label as given).
//                                           Computed once per line, shared by its n hypotheses.
//   kernel 2  sweep, backtrace, scores    : one wave per (line b, hypothesis q); workgroups never talk to each other.
//
// The sweep is a chain of lens[b] dependent steps.  Two recursions share the lattice: max (Viterbi) with a back pointer per (t, s),
// and logsumexp (the forward score, the lse3 of ctc_math.h, as in the alpha/beta sweeps of ctc.hip).
// TIE RULE of the Viterbi recursion: among equal predecessors prefer s, then s-1, then s-2 (a predecessor replaces the current
// choice only when STRICTLY greater); at the last frame the final blank 2L wins over 2L-1 on equality.
//   S <= 64 : one extended position per lane, both previous rows in registers, neighbours by wave shuffles, the frame's gathered
//             log-probability (which does not depend on the recursion) prefetched PF frames ahead.  No LDS row, no barrier.
//   S  > 64 : both previous rows in LDS (in the workspace beyond 1663 labels, where they no longer fit), lanes over 64-position chunks, updated in place from the highest chunk down (a chunk reads
//             only positions that no earlier chunk of the step wrote); the gathered log-probabilities of TB frames are staged into LDS
//             in one pass of independent loads, so the L2 round trip is paid once per TB frames.
// The recursion is the one of ctc_label_sweep (ctc_lattice.h) - the template over a cell type that the edit scores and the n-best
// gradient run over SumCell and the alignment entropy over its (a, e) cell - with the Viterbi row and its back pointers beside the
// sum.  It is written out here and not an instantiation of that template: as one, the S > 64 loop compiled to the same
// instructions at another address and ran 1.4 % slower (profiles/ctc_labelling_ab.txt has the kept form's figures).  PF, TB, the
// LDS size and the host side in front of the call are the header's.
// Back pointers take 2 bits per (t, s): two wave ballots (bit 0, bit 1) per (t, 64-position chunk), 16 bytes, written by lane 0.
// They live in LDS when the line's frames * chunks * 16 bytes fit beside the rows, else in the workspace.  The backtrace is serial (lane 0, one
// 16-byte read per frame); it yields for label p the first and last frame spent in state 2p+1.  Label scores (peak / sum of the
// class's frame log-probability over the span) are then computed by lane p % 64 in frame order.
// Every float is computed by a fixed lane in a fixed order and the only cross-lane operations are shuffles and ballots: results are
// bit-identical from run to run.
#include "ctc_lattice.h"

namespace {

struct BackPtr {
    ulonglong2* lds;
    ulonglong2* glob;
    __device__ __forceinline__ void put(long i, unsigned long long b0, unsigned long long b1) const {
        const ulonglong2 w = make_ulonglong2(b0, b1);
        if (lds) lds[i] = w; else glob[i] = w;
    }
    __device__ __forceinline__ int get(long i, int bit) const {
        const ulonglong2 w = lds ? lds[i] : glob[i];
        return (int)((w.x >> bit) & 1ull) | ((int)((w.y >> bit) & 1ull) << 1);
    }
};

// grid.x = B * n, 64 threads.  Dynamic LDS: [rows and staging of the S > 64 path: rows_floats floats][bp_lds_words 16-byte back-pointer
// words]; a problem whose lens[b] * chunks words do not fit there keeps them in its slice of bp_ws.
// ROWS_GLOBAL: the rows do not fit the LDS (more than 1663 labels) and live in the problem's slice of rows_ws instead.
template <bool ROWS_GLOBAL>
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ clp, const int32_t* __restrict__ lens,
                                                       const int32_t* __restrict__ canon, const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ label_lens, int T, int B, int V, int n,
                                                       int label_stride, int max_label_len, int SP, int rows_floats, int bp_lds_words,
                                                       ulonglong2* __restrict__ bp_ws, float* __restrict__ rows_ws,
                                                       float* __restrict__ out_scores,
                                                       int32_t* __restrict__ out_spans, float* __restrict__ out_label_scores) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x;
    const int prob = blockIdx.x, b = prob / n;
    const int len = min(max(lens[b], 0), T);
    const int L = label_lens[prob];
    const int32_t* lab = labels + (long)prob * label_stride;
    float* sc = out_scores + (long)prob * 2;
    int32_t* spans = out_spans + (long)prob * max_label_len * 2;
    float* lsc = out_label_scores + (long)prob * max_label_len * 2;
    const long tstride = (long)B * V;
    const float* lpb = clp + (long)b * V;                       // lpb[t * tstride + v]

    const bool bad = labelling_bad(canon, lab, L, V, max_label_len, lane);          // it cannot be aligned
    const int S = 2 * L + 1;
    float vit = NEG_INF, fwd = NEG_INF;
    int s_end = 0;
    const int NC = bad ? 1 : (S + 63) >> 6;
    BackPtr bp;
    bp.lds = (long)len * NC <= bp_lds_words ? (ulonglong2*)(sm + (ROWS_GLOBAL ? 0 : rows_floats)) : nullptr;
    bp.glob = bp_ws + (long)prob * T * (SP >> 6);

    if (bad || len == 0) {
        if (!bad && L == 0) vit = fwd = 0.f;
    } else if (S <= 64) {
        const bool in = lane < S;
        const int e = (in && (lane & 1)) ? lab[lane >> 1] : 0;
        const int c = class_of(canon, e);
        const int c_m2 = __shfl_up(c, 2, 64);
        const bool skip = lane >= 2 && e != 0 && c != c_m2;
        const float* col = lpb + e;
        float vm = NEG_INF;
        if (lane == 0 || (lane == 1 && S > 1)) vm = col[0];
        float vs = vm;
        float buf[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) buf[k] = col[(long)min(1 + k, len - 1) * tstride];
        for (int t0 = 1; t0 < len; t0 += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const int t = t0 + k;
                if (t < len) {                                   // wave-uniform
                    const float lpe = buf[k];
                    buf[k] = col[(long)min(t + PF, len - 1) * tstride];
                    float m2 = __shfl_up(vm, 1, 64), m3 = __shfl_up(vm, 2, 64);
                    float a2 = __shfl_up(vs, 1, 64), a3 = __shfl_up(vs, 2, 64);
                    if (lane < 1) { m2 = NEG_INF; a2 = NEG_INF; }
                    if (!skip) { m3 = NEG_INF; a3 = NEG_INF; }
                    float best = vm;
                    int from = 0;
                    if (m2 > best) { best = m2; from = 1; }
                    if (m3 > best) { best = m3; from = 2; }
                    const float l = lse3(vs, a2, a3);
                    vm = (in && best != NEG_INF) ? best + lpe : NEG_INF;
                    vs = (in && l != NEG_INF) ? l + lpe : NEG_INF;
                    const unsigned long long b0 = __ballot(from & 1), b1 = __ballot(from & 2);
                    if (lane == 0) bp.put(t, b0, b1);
                }
            }
        }
        const float am = __shfl(vm, S - 1, 64), cm = S > 1 ? __shfl(vm, S - 2, 64) : NEG_INF;
        const float as = __shfl(vs, S - 1, 64), cs = S > 1 ? __shfl(vs, S - 2, 64) : NEG_INF;
        s_end = cm > am ? S - 2 : S - 1;
        vit = fmaxf(am, cm);
        fwd = lse2(as, cs);
    } else {
        // rows with 2 leading -inf pads: rm[2 + s], rs[2 + s]; ext[s] = label | class << 16; em[k][s] the staged log-probabilities
        float* rows = ROWS_GLOBAL ? rows_ws + (long)prob * rows_floats : sm;
        float* rm = rows;
        float* rs = rows + (SP + 2);
        int* ext = (int*)(rows + 2 * (SP + 2));
        float* em = rows + 2 * (SP + 2) + SP;
        for (int s = lane; s < S; s += 64) {
            const int e = (s & 1) ? lab[s >> 1] : 0;
            ext[s] = e | (class_of(canon, e) << 16);
            float v = NEG_INF;
            if (s < 2) v = lpb[e];
            rm[2 + s] = v;
            rs[2 + s] = v;
        }
        if (lane < 2) { rm[lane] = NEG_INF; rs[lane] = NEG_INF; }
        __syncthreads();
        for (int t0 = 1; t0 < len; t0 += TB) {
            const int nk = min(TB, len - t0);
            for (int s = lane; s < S; s += 64) {
                const float* col = lpb + (ext[s] & 0xffff);
#pragma unroll
                for (int k = 0; k < TB; ++k)
                    if (k < nk) em[k * SP + s] = col[(long)(t0 + k) * tstride];
            }
            __syncthreads();
            for (int k = 0; k < nk; ++k) {
                const int t = t0 + k;
                for (int ch = NC - 1; ch >= 0; --ch) {
                    const int s = ch * 64 + lane;
                    const bool in = s < S;
                    float nm = NEG_INF, ns = NEG_INF;
                    int from = 0;
                    if (in) {
                        const int x = ext[s];
                        const bool skip = s >= 2 && (x & 0xffff) != 0 && (x >> 16) != (ext[s - 2] >> 16);
                        const float lpe = em[k * SP + s];
                        const float m1 = rm[2 + s], m2 = rm[1 + s], m3 = skip ? rm[s] : NEG_INF;
                        const float a1 = rs[2 + s], a2 = rs[1 + s], a3 = skip ? rs[s] : NEG_INF;
                        float best = m1;
                        if (m2 > best) { best = m2; from = 1; }
                        if (m3 > best) { best = m3; from = 2; }
                        const float l = lse3(a1, a2, a3);
                        nm = (best != NEG_INF) ? best + lpe : NEG_INF;
                        ns = (l != NEG_INF) ? l + lpe : NEG_INF;
                    }
                    const unsigned long long b0 = __ballot(from & 1), b1 = __ballot(from & 2);
                    if (in) { rm[2 + s] = nm; rs[2 + s] = ns; }
                    if (lane == 0) bp.put((long)t * NC + ch, b0, b1);
                }
                __syncthreads();
            }
        }
        const float am = rm[2 + S - 1], cm = rm[2 + S - 2];
        const float as = rs[2 + S - 1], cs = rs[2 + S - 2];
        s_end = cm > am ? S - 2 : S - 1;
        vit = fmaxf(am, cm);
        fwd = lse2(as, cs);
    }

    if (vit == NEG_INF) fwd = NEG_INF;                          // no path: both scores -inf
    if (lane == 0) { sc[0] = vit; sc[1] = fwd; }
    const bool aligned = vit != NEG_INF && len > 0;
    const int nlab = aligned ? L : 0;
    for (int p = nlab + lane; p < max_label_len; p += 64) {
        spans[2 * p] = -1; spans[2 * p + 1] = -1;
        lsc[2 * p] = 0.f; lsc[2 * p + 1] = 0.f;
    }
    if (nlab == 0) return;

    // backtrace (lane 0): every label of a feasible path is visited, so every span below L is written exactly once
    if (lane == 0) {
        int s = s_end, run_last = len - 1;
        for (int t = len - 1; t >= 1; --t) {
            const int from = bp.get((long)t * NC + (s >> 6), s & 63);
            if (from) {
                if (s & 1) { spans[s - 1] = t; spans[s] = run_last; }          // label p = (s-1)/2: spans[2p], spans[2p+1]
                s = max(s - from, 0);
                run_last = t - 1;
            }
        }
        if (s & 1) { spans[s - 1] = 0; spans[s] = run_last; }
    }
    __syncthreads();
    for (int p = lane; p < L; p += 64) {
        const int first = spans[2 * p], last = spans[2 * p + 1];
        float peak = 0.f, sum = 0.f;
        if (first >= 0 && last >= first && last < len) {
            const float* col = lpb + lab[p];
            peak = NEG_INF;
            for (int t = first; t <= last; ++t) {
                const float x = col[(long)t * tstride];
                peak = fmaxf(peak, x);
                sum += x;
            }
        }
        lsc[2 * p] = peak;
        lsc[2 * p + 1] = sum;
    }
}

struct Plan {
    int sp;                // extended positions rounded up to 64
    size_t rows_floats;    // floats of the S > 64 path's rows and staging (0 when every labelling fits one wave)
    size_t bp_bytes;       // back pointers of one (line, hypothesis)
    bool rows_lds;         // the rows fit the LDS (up to 1663 labels)
    bool bp_lds;           // ... and the longest line's back pointers beside them
    bool ok;
};

Plan align_plan(int t, int b, int v, int n, int max_label_len) {
    Plan p = {0, 0, 0, false, false, false};
    const LabelPlan lp = label_plan(t, b, v, n, max_label_len);
    if (!lp.ok || (long)b * n * (max_label_len > 0 ? max_label_len : 1) * 2 >= (1L << 31)) return p;
    p.sp = lp.sp;
    p.rows_floats = (sweep_floats(p.sp, 2) + 3) & ~(size_t)3;    // the back pointers behind them are 16-byte words
    p.rows_lds = p.rows_floats * 4 <= LDS_BUDGET;
    p.bp_bytes = (size_t)t * (p.sp / 64) * 16;
    p.bp_lds = (p.rows_lds ? p.rows_floats * 4 : 0) + p.bp_bytes <= LDS_BUDGET;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t vocr_ctc_align_workspace_bytes(int t, int b, int v, int n, int max_label_len) {
    const Plan p = align_plan(t, b, v, n, max_label_len);
    if (!p.ok) return 0;
    return clp_bytes(t, b, v) + (p.bp_lds ? 0 : (size_t)b * n * p.bp_bytes) + (p.rows_lds ? 0 : (size_t)b * n * p.rows_floats * 4);
}

extern "C" int vocr_ctc_align(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                              const int32_t* labels, const int32_t* label_lens, int n, int label_stride, int max_label_len,
                              float* out_scores, int32_t* out_spans, float* out_label_scores, void* workspace, size_t workspace_bytes,
                              void* stream) {
    const char* who = "vocr_ctc_align";
    VOCR_CHECK_ARG(logits && lens && labels && label_lens && out_scores && out_spans && out_label_scores && workspace, "%s: null pointer",
                   who);
    if (check_labelling_shape(who, t, b, v, n, label_stride, max_label_len) != VOCR_OK) return VOCR_EINVAL;
    const Plan p = align_plan(t, b, v, n, max_label_len);
    VOCR_CHECK_ARG(p.ok, "vocr_ctc_align: unsupported shape (t=%d b=%d v=%d n=%d max_label_len=%d): t*b*n or b*n*max_label_len too large",
                   t, b, v, n, max_label_len);
    const size_t need = vocr_ctc_align_workspace_bytes(t, b, v, n, max_label_len);
    VOCR_CHECK_ARG(workspace_bytes >= need, "vocr_ctc_align: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    static VocrPerDevice lds_set;
    const void* const big[] = {(const void*)ctc_align_kernel<false>, (const void*)ctc_align_kernel<true>};
    if (vocr_allow_dynamic_lds(big, 2, (int)LDS_BUDGET, &lds_set, who) != VOCR_OK) return VOCR_ELAUNCH;
    float* clp = (float*)workspace;
    ulonglong2* bp_ws = (ulonglong2*)((char*)workspace + clp_bytes(t, b, v));
    VOCR_CHECK_ARG(p.bp_lds || (((uintptr_t)workspace) & 15) == 0, "vocr_ctc_align: workspace must be 16-byte aligned");
    if (launch_class_logprob(who, logits, lens, canon, clp, t, b, v, s) != VOCR_OK) return VOCR_ELAUNCH;
    // where the longest line's back pointers do not fit, shorter lines still keep theirs in what is left of 64 KiB (two lines per CU)
    const size_t rows_bytes = p.rows_lds ? p.rows_floats * 4 : 0;
    const size_t bp_lds = p.bp_lds ? p.bp_bytes : (rows_bytes < 64 * 1024 ? 64 * 1024 - rows_bytes : 0);
    const size_t lds = rows_bytes + bp_lds;
    float* rows_ws = (float*)((char*)bp_ws + (p.bp_lds ? 0 : (size_t)b * n * p.bp_bytes));
    if (p.rows_lds)
        ctc_align_kernel<false><<<b * n, 64, lds, s>>>(clp, lens, canon, labels, label_lens, t, b, v, n, label_stride, max_label_len, p.sp,
                                                       (int)p.rows_floats, (int)(bp_lds / 16), bp_ws, rows_ws, out_scores, out_spans,
                                                       out_label_scores);
    else
        ctc_align_kernel<true><<<b * n, 64, lds, s>>>(clp, lens, canon, labels, label_lens, t, b, v, n, label_stride, max_label_len, p.sp,
                                                      (int)p.rows_floats, (int)(bp_lds / 16), bp_ws, rows_ws, out_scores, out_spans,
                                                      out_label_scores);
    VOCR_CHECK_LAUNCH("vocr_ctc_align(sweep)");
    return VOCR_OK;
}
