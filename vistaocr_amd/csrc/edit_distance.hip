// Edit statistics of hypotheses against references: what compute_cer_wer (src/textutils.py:326-351) and src/edit_dist_trace.py compute
// on the host, for a list of (hypothesis, reference) pairs that never leave the device.  Integer arithmetic only: every output is
// bit for bit the cell-by-cell DP's.
//
//   D[i][0] = i, D[0][j] = j,   D[i][j] = min(D[i-1][j-1] + (A_i != B_j), D[i-1][j] + 1, D[i][j-1] + 1)
//
// A (rows, i) is the hypothesis, B (columns, j) the reference.  TIE RULE of the trace (edit_dist_trace.py): at a cell take the diagonal
// (COPY when the elements are equal, else SUB) if its cost is <= both others, otherwise INS (from i-1) if its cost is <= DEL's,
// otherwise DEL (from j-1).  The walk starts at (|A|, |B|) and is complete: at j = 0 what is left of A is INS, at i = 0 what is left of
// B is DEL.
//
// One wave per pair, persistent: workgroup g of G (one wave each) takes pairs g, g + G, ..  The reference's columns are cut into blocks
// of 64, lane l owns column 64 * blk + l of the block and walks down its rows on the anti-diagonal: at step k it computes row k - l
// from its own previous value (i-1, j), the value its left neighbour computed one step ago (i, j-1: ONE lane shift per step) and the
// one it received the step before (i-1, j-1: kept in a register).  Lane 0's left neighbour is the previous block's last column, which
// lane 63 leaves in an LDS column as it goes (read at index k, written at index k - 63: in place).  With the trace asked for every lane
// packs the 2-bit operation of 16 consecutive rows of its column into a dword and stores it at [row / 16][column]: in the LDS where
// the pair's table fits (BP_LDS dwords), else in the workgroup's own slab of the workspace - per resident workgroup, not per pair.
// Lane 0 walks the table backwards, counts the operations, adds them to the confusion matrix with integer atomics and leaves the
// operation codes in the LDS; the wave writes them out from the front.
//
// Words (form_tokenized_words, src/textutils.py:290-323) are formed on the device from the classes' kinds: a run of letters is one
// token, every single (punctuation mark, digit) a token of its own, anything else separates.  64 characters at a time, a ballot
// numbers the token starts and the lane at a start measures and hashes its token.  Two tokens are equal iff they have the same length
// and the same classes (the hash only pre-filters); the word statistics are the same recursion and the same walk over the tokens.
//
// No floating point and a fixed lane for every cell: results are bit-identical from run to run (the confusion matrix is a sum of
// integer atomics).
#include "ctc_align_common.h"

namespace {

constexpr int LEN_MAX = 2048;                // characters per side (the limit the header states)
constexpr int BP_LDS = 8192;                 // dwords of back pointers kept in the LDS (a 256 x 512 pair; 32 KiB)
constexpr int G_TRACE = 256;                 // workgroups with back pointers (50 KiB of LDS, 83 KiB with words: 3 and 1 per CU), one per
                                             // CU: each owns a slab of the workspace
constexpr int G_TRACE_LDS = 256;             // with back pointers that all fit the LDS (no slab)
constexpr bool SHIFT_DPP = false;            // the lane shift of the recursion (from_left)
constexpr int G_DIST = 2048;                 // without: workgroups in the grid (13 KiB of LDS each for characters, 46 KiB with words:
                                             // 12 and 3 of them per CU are resident at a time, the rest queue behind them)
constexpr int KIND_LETTER = 1, KIND_SINGLE = 3;               // as vocr_ctc_word_beam_search's cls_kind (2 = space: a separator)
constexpr int OP_COPY = 1, OP_SUB = 2, OP_INS = 3, OP_DEL = 4;
constexpr int WANT_CHARS = 1, WANT_WORDS = 2, WANT_TRACE = 4;
constexpr int NSTAT = 12;

__host__ __device__ inline int pad64(int n) { return (n + 63) & ~63; }

// lane l receives lane l - 1's value (lane 0's is not used): a DPP wave_shr:1 on the VALU, or __shfl_up's ds_bpermute through the LDS
// crossbar.  It sits in the recursion's dependent chain.
template <bool DPP>
__device__ __forceinline__ int from_left(int v) {
    if (DPP) return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false);
    return __shfl_up(v, 1, 64);
}

// the elements of a DP: neq(i0) compares row i0 with the column the lane holds
struct CharSide {
    const uint8_t* a;
    const uint8_t* b;
    int bc;
    __device__ __forceinline__ void load_col(int c0, bool ok) { bc = ok ? b[c0] : -1; }
    __device__ __forceinline__ bool neq(int i0) const { return a[i0] != bc; }
};

struct Tokens {
    const uint8_t* cls;
    const uint16_t* pos;
    const uint16_t* len;
    const uint32_t* hash;
};

struct WordSide {
    Tokens a, b;
    int bpos, blen;
    uint32_t bhash;
    __device__ __forceinline__ void load_col(int c0, bool ok) {
        bpos = ok ? b.pos[c0] : 0;
        blen = ok ? b.len[c0] : -1;
        bhash = ok ? b.hash[c0] : 0;
    }
    __device__ __forceinline__ bool neq(int i0) const {
        if (a.len[i0] != blen || a.hash[i0] != bhash) return true;
        const int ap = a.pos[i0];
        for (int k = 0; k < blen; ++k)
            if (a.cls[ap + k] != b.cls[bpos + k]) return true;
        return false;
    }
};

// D[la][lb] by the whole wave (uniform result).  bnd: la + 1 ints of LDS.  TRACE: bp[(i-1) / 16][ldb] receives the operations.
template <bool TRACE, bool DPP, class Side>
__device__ __forceinline__ int wave_dp(Side& sd, int la, int lb, int* bnd, uint32_t* bp, int ldb) {
    const int lane = threadIdx.x;
    if (la == 0 || lb == 0) return la + lb;                       // the walk needs no table there
    for (int i = lane; i <= la; i += 64) bnd[i] = i;              // column 0
    __syncthreads();
    int result = 0;
    const int nblk = (lb + 63) >> 6;
    for (int blk = 0; blk < nblk; ++blk) {
        const int c0 = blk * 64 + lane;                           // 0-based column
        const bool colok = c0 < lb;
        sd.load_col(c0, colok);
        int cur = c0 + 1;                                         // D[0][c0 + 1]
        int keep = c0;                                            // D[0][c0]: the diagonal of row 1 (bnd[0] is never read)
        uint32_t acc = 0;
        const int nsteps = la + min(64, lb - blk * 64) - 1;
        for (int k = 1; k <= nsteps; ++k) {
            int left = from_left<DPP>(cur);
            if (lane == 0) left = bnd[min(k, la)];
            const int i = k - lane;
            const int diag = keep;
            keep = left;
            if (colok && i >= 1 && i <= la) {
                const bool ne = sd.neq(i - 1);
                const int sub = diag + (ne ? 1 : 0), ins = cur + 1, del = left + 1;
                int op;
                if (sub <= ins && sub <= del) {
                    cur = sub;
                    op = ne ? OP_SUB : OP_COPY;
                } else if (ins <= del) {
                    cur = ins;
                    op = OP_INS;
                } else {
                    cur = del;
                    op = OP_DEL;
                }
                if (lane == 63) bnd[i] = cur;
                if (TRACE) {
                    const int sh = (i - 1) & 15;
                    acc |= (uint32_t)(op - 1) << (2 * sh);
                    if (sh == 15 || i == la) {
                        bp[(long)((i - 1) >> 4) * ldb + c0] = acc;
                        acc = 0;
                    }
                }
            }
        }
        if (blk == nblk - 1) result = __shfl(cur, (lb - 1) & 63, 64);
        __syncthreads();                                          // lane 63's column, for the next block's lane 0
    }
    return result;
}

// one lane: from (la, lb) back to (0, 0); emit(op, i, j) for every operation, last one first
template <class Emit>
__device__ __forceinline__ void walk_back(int la, int lb, const uint32_t* bp, int ldb, int& nsub, int& nins, int& ndel, Emit&& emit) {
    int i = la, j = lb;
    while (i > 0 || j > 0) {
        int op;
        if (j == 0) op = OP_INS;
        else if (i == 0) op = OP_DEL;
        else op = (int)((bp[(long)((i - 1) >> 4) * ldb + (j - 1)] >> (2 * ((i - 1) & 15))) & 3u) + 1;
        emit(op, i, j);
        if (op == OP_INS) {
            --i;
            ++nins;
        } else if (op == OP_DEL) {
            --j;
            ++ndel;
        } else {
            --i;
            --j;
            nsub += op == OP_SUB ? 1 : 0;
        }
    }
}

// the tokens of cls[0 .. L) by the whole wave; returns their number (uniform)
__device__ __forceinline__ int tokenize(const uint8_t* cls, int L, const uint8_t* kind, uint16_t* tpos, uint16_t* tlen, uint32_t* thash) {
    const int lane = threadIdx.x;
    int ntok = 0;
    for (int base = 0; base < L; base += 64) {
        const int pos = base + lane;
        const int k = pos < L ? kind[cls[pos]] : 0;
        const int kp = (pos > 0 && pos < L) ? kind[cls[pos - 1]] : 0;
        const bool start = k == KIND_SINGLE || (k == KIND_LETTER && kp != KIND_LETTER);
        const unsigned long long m = __ballot(start);
        if (start) {
            const int idx = ntok + __popcll(m & ((1ull << lane) - 1ull));
            int len = 1;
            uint32_t h = (2166136261u ^ cls[pos]) * 16777619u;
            if (k == KIND_LETTER)
                while (pos + len < L && kind[cls[pos + len]] == KIND_LETTER) {
                    h = (h ^ cls[pos + len]) * 16777619u;
                    ++len;
                }
            tpos[idx] = (uint16_t)pos;
            tlen[idx] = (uint16_t)len;
            thash[idx] = h;
        }
        ntok += __popcll(m);
    }
    return ntok;
}

// classes of labels[0 .. L) into dst; true (on some lane) where a label is <= 0, >= V or in the blank's class
__device__ __forceinline__ bool load_classes(const int32_t* __restrict__ labels, int L, const int* s_cls, int V, uint8_t* dst) {
    bool bad = false;
    for (int i = threadIdx.x; i < L; i += 64) {
        const int v = labels[i];
        const bool out = v <= 0 || v >= V;
        const int c = s_cls[out ? 0 : v];
        bad |= out || c == 0;
        dst[i] = (uint8_t)c;
    }
    return bad;
}

// grid.x = resident workgroups, 64 threads.  slab: slab_dwords per workgroup (TRACE, pairs whose table does not fit the LDS).
template <bool WORDS, bool TRACE, bool DPP>
__global__ __launch_bounds__(64) void edit_stats_kernel(const int32_t* __restrict__ a_labels, const int32_t* __restrict__ a_lens, int na,
                                                        int a_stride, int max_a, const int32_t* __restrict__ b_labels,
                                                        const int32_t* __restrict__ b_lens, int nb, int b_stride, int max_b,
                                                        const int32_t* __restrict__ pairs, int np, const int32_t* __restrict__ canon,
                                                        const int32_t* __restrict__ kinds, int V, int want,
                                                        int32_t* __restrict__ out_stats, int32_t* __restrict__ out_confusion,
                                                        uint8_t* __restrict__ out_ops, int ops_stride, uint32_t* __restrict__ slab,
                                                        long slab_dwords) {
    __shared__ int s_cls[VMAX];
    __shared__ uint8_t s_kind[WORDS ? VMAX : 4];
    __shared__ uint8_t s_a[LEN_MAX], s_b[LEN_MAX];
    __shared__ int s_bnd[LEN_MAX + 1];
    __shared__ uint16_t s_tpos[2][WORDS ? LEN_MAX : 2], s_tlen[2][WORDS ? LEN_MAX : 2];
    __shared__ uint32_t s_thash[2][WORDS ? LEN_MAX : 1];
    __shared__ uint32_t s_bp[TRACE ? BP_LDS : 1];
    __shared__ uint8_t s_ops[TRACE ? 2 * LEN_MAX : 4];
    __shared__ int s_nops;
    const int lane = threadIdx.x;
    for (int v = lane; v < V; v += 64) {
        const int c = class_of(canon, v);
        s_cls[v] = c;
        if (WORDS) {
            const int k = kinds[c];
            s_kind[v] = (uint8_t)((k == KIND_LETTER || k == KIND_SINGLE) ? k : 0);
        }
    }
    uint32_t* my_slab = (TRACE && slab) ? slab + (long)blockIdx.x * slab_dwords : nullptr;

    for (int p = blockIdx.x; p < np; p += gridDim.x) {
        __syncthreads();                                          // the tables above; the previous pair's readers
        const int ia = pairs[2 * (long)p], ib = pairs[2 * (long)p + 1];
        bool bad = ia < 0 || ia >= na || ib < 0 || ib >= nb;
        int la = 0, lb = 0;
        if (!bad) {
            la = a_lens[ia];
            lb = b_lens[ib];
            bad = la < 0 || la > max_a || lb < 0 || lb > max_b;
        }
        if (!bad) {                                               // uniform
            bool lbad = load_classes(a_labels + (long)ia * a_stride, la, s_cls, V, s_a);
            lbad |= load_classes(b_labels + (long)ib * b_stride, lb, s_cls, V, s_b);
            bad = __any(lbad);
        }
        int32_t* st = out_stats + (long)NSTAT * p;
        uint8_t* ops_row = (TRACE && out_ops) ? out_ops + (long)p * ops_stride : nullptr;
        if (bad) {
            if (lane < NSTAT) st[lane] = -1;
            if (ops_row)
                for (int t = lane; t < ops_stride; t += 64) ops_row[t] = 0;
            continue;
        }
        __syncthreads();
        int stat[NSTAT];
#pragma unroll
        for (int k = 0; k < NSTAT; ++k) stat[k] = -1;

        if (want & WANT_CHARS) {
            CharSide cs = {s_a, s_b, 0};
            const int ldb = pad64(lb);
            uint32_t* bp = nullptr;
            if (TRACE) bp = (long)((la + 15) >> 4) * ldb <= BP_LDS ? s_bp : my_slab;
            stat[0] = wave_dp<TRACE, DPP>(cs, la, lb, s_bnd, bp, ldb);
            stat[4] = la;
            stat[5] = lb;
            if (TRACE) {
                __syncthreads();                                  // the table is complete, in the LDS or in memory
                if (lane == 0) {
                    int nsub = 0, nins = 0, ndel = 0, nops = 0;
                    walk_back(la, lb, bp, ldb, nsub, nins, ndel, [&](int op, int i, int j) {
                        s_ops[nops++] = (uint8_t)op;
                        if (out_confusion) {
                            const int r = op == OP_INS ? 0 : s_b[j - 1], h = op == OP_DEL ? 0 : s_a[i - 1];
                            atomicAdd(out_confusion + r * V + h, 1);
                        }
                    });
                    stat[1] = nsub;
                    stat[2] = nins;
                    stat[3] = ndel;
                    s_nops = nops;
                }
                __syncthreads();
                if (ops_row) {
                    const int nops = s_nops;
                    for (int t = lane; t < ops_stride; t += 64) ops_row[t] = t < nops ? s_ops[nops - 1 - t] : (uint8_t)0;
                }
            }
        }

        if (WORDS && (want & WANT_WORDS)) {
            const int wa = tokenize(s_a, la, s_kind, s_tpos[0], s_tlen[0], s_thash[0]);
            const int wb = tokenize(s_b, lb, s_kind, s_tpos[1], s_tlen[1], s_thash[1]);
            __syncthreads();
            WordSide ws = {{s_a, s_tpos[0], s_tlen[0], s_thash[0]}, {s_b, s_tpos[1], s_tlen[1], s_thash[1]}, 0, 0, 0};
            const int ldb = pad64(wb);
            uint32_t* bp = nullptr;
            if (TRACE) bp = (long)((wa + 15) >> 4) * ldb <= BP_LDS ? s_bp : my_slab;
            stat[6] = wave_dp<TRACE, DPP>(ws, wa, wb, s_bnd, bp, ldb);
            stat[10] = wa;
            stat[11] = wb;
            if (TRACE) {
                __syncthreads();
                if (lane == 0) {
                    int nsub = 0, nins = 0, ndel = 0;
                    walk_back(wa, wb, bp, ldb, nsub, nins, ndel, [](int, int, int) {});
                    stat[7] = nsub;
                    stat[8] = nins;
                    stat[9] = ndel;
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NSTAT; ++k) st[k] = stat[k];
        }
    }
}

struct Plan {
    long slab_dwords;      // back pointers of one resident workgroup in the workspace (0: every pair fits the LDS, or no trace)
    int groups;            // resident workgroups
    bool ok;
};

Plan plan_for(int na, int nb, int np, int v, int max_a_len, int max_b_len, int want) {
    Plan p = {0, 0, false};
    if (na < 1 || nb < 1 || np < 1 || v < 2 || v > VMAX) return p;
    if (max_a_len < 0 || max_a_len > LEN_MAX || max_b_len < 0 || max_b_len > LEN_MAX) return p;
    if (!(want & (WANT_CHARS | WANT_WORDS)) || (want & ~(WANT_CHARS | WANT_WORDS | WANT_TRACE))) return p;
    if ((want & WANT_TRACE) && !(want & WANT_CHARS)) return p;    // the trace is the characters'
    p.ok = true;
    if (want & WANT_TRACE) {
        const long table = (long)((max_a_len + 15) >> 4) * pad64(max_b_len);
        p.slab_dwords = table > BP_LDS ? table : 0;
        const int g = p.slab_dwords ? G_TRACE : VOCR_EXPERIMENT_INT("VOCR_ES_GTRACE_LDS", G_TRACE_LDS);    // no slab: nothing to own
        p.groups = np < g ? np : g;
    } else {
        p.groups = np < G_DIST ? np : G_DIST;
    }
    return p;
}

}  // namespace

extern "C" size_t vocr_edit_stats_workspace_bytes(int na, int nb, int np, int v, int max_a_len, int max_b_len, int want) {
    const Plan p = plan_for(na, nb, np, v, max_a_len, max_b_len, want);
    if (!p.ok) return 0;
    return 16 + (size_t)p.groups * (size_t)p.slab_dwords * sizeof(uint32_t);
}

extern "C" int vocr_edit_stats(const int32_t* a_labels, const int32_t* a_lens, int na, int a_stride, int max_a_len,
                               const int32_t* b_labels, const int32_t* b_lens, int nb, int b_stride, int max_b_len,
                               const int32_t* pairs, int np, const int32_t* canon, const int32_t* kinds, int v, int want,
                               int32_t* out_stats, int32_t* out_confusion, uint8_t* out_ops, int ops_stride,
                               void* workspace, size_t workspace_bytes, void* stream) {
    VOCR_CHECK_ARG(na >= 1 && nb >= 1 && np >= 1, "vocr_edit_stats: need na >= 1, nb >= 1, np >= 1 (na=%d nb=%d np=%d)", na, nb, np);
    VOCR_CHECK_ARG(v >= 2 && v <= VMAX, "vocr_edit_stats: need 2 <= v <= %d (v=%d)", VMAX, v);
    VOCR_CHECK_ARG(max_a_len >= 0 && max_a_len <= LEN_MAX && max_b_len >= 0 && max_b_len <= LEN_MAX,
                   "vocr_edit_stats: need 0 <= max_a_len, max_b_len <= %d (max_a_len=%d max_b_len=%d)", LEN_MAX, max_a_len, max_b_len);
    VOCR_CHECK_ARG(a_stride >= max_a_len && b_stride >= max_b_len && a_stride >= 0 && b_stride >= 0,
                   "vocr_edit_stats: need a_stride >= max_a_len and b_stride >= max_b_len (a_stride=%d max_a_len=%d b_stride=%d max_b_len=%d)",
                   a_stride, max_a_len, b_stride, max_b_len);
    const Plan p = plan_for(na, nb, np, v, max_a_len, max_b_len, want);
    VOCR_CHECK_ARG(p.ok, "vocr_edit_stats: unsupported want=%d: bit 0 (characters) or bit 1 (words) must be set, bit 2 (trace) needs bit 0, "
                   "no other bit", want);
    VOCR_CHECK_ARG(a_labels && a_lens && b_labels && b_lens && pairs && out_stats && workspace, "vocr_edit_stats: null pointer");
    VOCR_CHECK_ARG(!out_ops || ((want & WANT_TRACE) && ops_stride >= max_a_len + max_b_len),
                   "vocr_edit_stats: out_ops needs want bit 2 and ops_stride >= max_a_len + max_b_len (ops_stride=%d)", ops_stride);
    VOCR_CHECK_ARG(!out_confusion || (want & WANT_TRACE), "vocr_edit_stats: out_confusion needs want bit 2");
    const size_t need = vocr_edit_stats_workspace_bytes(na, nb, np, v, max_a_len, max_b_len, want);
    VOCR_CHECK_ARG(workspace_bytes >= need, "vocr_edit_stats: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    uint32_t* slab = p.slab_dwords ? (uint32_t*)((char*)workspace + 16) : nullptr;
    const bool words = (want & WANT_WORDS) && kinds;
    const bool trace = want & WANT_TRACE;
    VOCR_CHECK_ARG(words || (want & WANT_CHARS), "vocr_edit_stats: want asks for words only and kinds is NULL: nothing to compute");
#define ES_ARGS a_labels, a_lens, na, a_stride, max_a_len, b_labels, b_lens, nb, b_stride, max_b_len, pairs, np, canon, kinds, v, want, \
                out_stats, out_confusion, out_ops, ops_stride, slab, p.slab_dwords
#define ES_LAUNCH(DPP)                                                                                  \
    if (words && trace) edit_stats_kernel<true, true, DPP><<<p.groups, 64, 0, s>>>(ES_ARGS);            \
    else if (words) edit_stats_kernel<true, false, DPP><<<p.groups, 64, 0, s>>>(ES_ARGS);               \
    else if (trace) edit_stats_kernel<false, true, DPP><<<p.groups, 64, 0, s>>>(ES_ARGS);               \
    else edit_stats_kernel<false, false, DPP><<<p.groups, 64, 0, s>>>(ES_ARGS);
#ifdef VOCR_EXPERIMENTS
    if (VOCR_EXPERIMENT_INT("VOCR_ES_DPP", SHIFT_DPP ? 1 : 0)) {
        ES_LAUNCH(true)
    } else {
        ES_LAUNCH(false)
    }
#else
    ES_LAUNCH(SHIFT_DPP)
#endif
#undef ES_LAUNCH
#undef ES_ARGS
    VOCR_CHECK_LAUNCH("vocr_edit_stats");
    return VOCR_OK;
}
