// Training augmentation of a collated line batch on the device: the chain the reference applies per image on the host
// (src/train_cnn_lstm.py:203-274, src/imagetransforms.py:71-406) as ONE gather over x[B][C][H][Wmax] with every line's width kept.
// All randomness arrives in per-line tables drawn on the host (include/vocr.h: the record layout); the kernels are a pure function
// of their arguments.  Per output pixel (b, ch, oy, ox < w_b):
//   1 geometry     p = (ox + Dx, oy + Dy), D the bilinear interpolation of the line's mesh node displacements (exactly 0 without the
//                  mesh flag); (xs, ys) = A_b (p, 1), clamped to [0, w-1] x [0, H-1] (border replicate); R = bilinear sample of
//                  x[b, ch], second tap min(i + 1, limit): no tap reads a column >= w_b.  All channels share the geometry.
//   2 block filter F = bias + sum k[i][j] R(oy-1+i, ox-1+j), R = 0 outside the line, then (F - min) / (max - min) over the whole line
//                  (0 when max = min).  min / max: pass 1 writes one (min, max) per workgroup into the workspace, pass 2 folds the
//                  line's partials again in every wave.  min and max do not depend on the order: bit-identical from run to run.
//   3 photometric  contrast, invert, noise, delete, stripe, clamp to [0, 1], in that order; the draws are counter-based
//                  (aug_bits below), a function of (line key, channel, oy, ox, draw) only.
//   4 padding      y[b, :, :, ox >= w_b] = 0.
// Launch shape: a workgroup is 256 lanes along the row x ROWS rows of one channel of one line; a lane walks down its column, so the
// 2x2 filter keeps the row above in registers (two geometry samples per pixel, not four).  Loads are plain global gathers: for the
// mild maps of the recipe neighbouring lanes read neighbouring addresses, stores are one contiguous row segment per step.
// Arithmetic is pinned: contraction is off and every fused multiply-add is written out, so that a value does not depend on where
// the compiler inlined its expression (a line alone and the same line inside a batch give the same bits).
#include "vocr_common.h"

namespace {

constexpr int TW = 256;          // lanes of a workgroup = columns of a tile
constexpr int ROWS = 8;          // rows of a tile
constexpr int REC = 24;          // 32-bit words of a line's record (include/vocr.h)
constexpr int DIM_MAX = 1 << 24; // h, wmax: a pixel's counter keeps 24 bits for each

#pragma clang fp contract(off)

struct Line {
    float a00, a01, a02, a10, a11, a12;
    float k00, k01, k10, k11, bias;
    float alpha, p_noise, sigma, p_del, del_value, stripe_value;
    int mesh, filter, invert, gw, r0, r1;
    uint64_t key;
};

__device__ __forceinline__ float word_f(const uint32_t* __restrict__ r, int i) { return __uint_as_float(r[i]); }

__device__ __forceinline__ Line load_line(const uint32_t* __restrict__ r, bool have_mesh, int gw_max, int with_filter) {
    Line L;
    L.a00 = word_f(r, 0), L.a01 = word_f(r, 1), L.a02 = word_f(r, 2);
    L.a10 = word_f(r, 3), L.a11 = word_f(r, 4), L.a12 = word_f(r, 5);
    L.k00 = word_f(r, 6), L.k01 = word_f(r, 7), L.k10 = word_f(r, 8), L.k11 = word_f(r, 9), L.bias = word_f(r, 10);
    L.alpha = word_f(r, 11), L.p_noise = word_f(r, 12), L.sigma = word_f(r, 13), L.p_del = word_f(r, 14);
    L.del_value = word_f(r, 15), L.stripe_value = word_f(r, 16);
    const uint32_t flags = r[17];
    L.mesh = (flags & 1u) && have_mesh;
    L.filter = (flags & 2u) && with_filter;
    L.invert = (flags & 4u) != 0;
    L.gw = min(max((int)r[18], 1), max(gw_max, 1));      // a record cannot lead outside the mesh table
    L.r0 = (int)r[19], L.r1 = (int)r[20];
    L.key = (uint64_t)r[21] | ((uint64_t)r[22] << 32);
    return L;
}

// the draw of (line key, channel, oy, ox, draw id): vocr_dropout_fwd's hash (the splitmix64 finaliser, upper 32 bits) of
// key * 0x9e3779b97f4a7c15 + counter, counter = ox | oy << 24 | ch << 48 | draw << 56
__device__ __forceinline__ uint32_t aug_bits(uint64_t key, int ch, int oy, int ox, int draw) {
    uint64_t z = key * 0x9e3779b97f4a7c15ull + ((uint64_t)ox | ((uint64_t)oy << 24) | ((uint64_t)ch << 48) | ((uint64_t)draw << 56));
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 32);
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return fmaf(t, b - a, a); }   // exactly a at t = 0

// Stage 1 at output pixel (ox, oy) of a line of width w >= 1.  xc = x[b][ch]; md = the line's mesh block (dx plane, dy plane behind
// it, each [gh + 1][gws]), only read with L.mesh
__device__ __forceinline__ float sample(const float* __restrict__ xc, int wmax, int h, int w, const Line& L, const float* __restrict__ md,
                                        int gh, int gws, float sx, float sy, int ox, int oy) {
    float px = (float)ox, py = (float)oy;
    if (L.mesh) {
        const float u = px * sx, v = py * sy;
        const int j = min((int)u, L.gw - 1), i = min((int)v, gh - 1);
        const float fu = u - (float)j, fv = v - (float)i;
        const float* m = md + i * gws + j;
        const float* n = m + (gh + 1) * gws;
        const float dx = lerp(lerp(m[0], m[1], fu), lerp(m[gws], m[gws + 1], fu), fv);
        const float dy = lerp(lerp(n[0], n[1], fu), lerp(n[gws], n[gws + 1], fu), fv);
        px += dx;
        py += dy;
    }
    float xs = fmaf(L.a00, px, fmaf(L.a01, py, L.a02));
    float ys = fmaf(L.a10, px, fmaf(L.a11, py, L.a12));
    xs = fminf(fmaxf(xs, 0.f), (float)(w - 1));          // fmaxf(NaN, 0) = 0: whatever the tables hold, the taps stay inside the line
    ys = fminf(fmaxf(ys, 0.f), (float)(h - 1));
    const int x0 = (int)xs, y0 = (int)ys;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float fx = xs - (float)x0, fy = ys - (float)y0;
    const float* r0 = xc + (size_t)y0 * wmax;
    const float* r1 = xc + (size_t)y1 * wmax;
    return lerp(lerp(r0[x0], r0[x1], fx), lerp(r1[x0], r1[x1], fx), fy);
}

// Stage 3 on a value v
__device__ __forceinline__ float photometric(float v, const Line& L, int ch, int oy, int ox) {
    const float U = 1.0f / 16777216.0f;
    if (L.alpha != 1.f) v = fmaf(v - 0.5f, L.alpha, 0.5f);            // alpha = 1 is skipped: v - 0.5 rounds for a small v
    if (L.invert) v = 1.f - v;
    if (L.p_noise > 0.f && (float)(aug_bits(L.key, ch, oy, ox, 0) >> 8) * U < L.p_noise) {
        const float u1 = (float)((aug_bits(L.key, ch, oy, ox, 1) >> 8) + 1u) * U;
        const float u2 = (float)(aug_bits(L.key, ch, oy, ox, 2) >> 8) * U;
        const float n = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        v = fmaf(L.sigma, n, v);
    }
    if (L.p_del > 0.f && (float)(aug_bits(L.key, ch, oy, ox, 3) >> 8) * U < L.p_del) v = L.del_value;
    if (oy >= L.r0 && oy < L.r1) v = L.stripe_value;
    return fminf(fmaxf(v, 0.f), 1.f);
}

// grid = (column tiles, c * row tiles, b), TW threads.  MINMAX: pass 1, one (min, max) of the filter's output per workgroup into
// part[b][blockIdx.y * gridDim.x + blockIdx.x] for every line with the filter flag.  Otherwise pass 2: everything, into y.
template <bool MINMAX>
__global__ __launch_bounds__(TW) void augment_kernel(const float* __restrict__ x, const int32_t* __restrict__ widths, int c, int h, int wmax,
                                                     const uint32_t* __restrict__ params, const float* __restrict__ mesh, int gh,
                                                     int gw_max, int with_filter, float* __restrict__ y, float2* __restrict__ part) {
    __shared__ float s_mn[TW / VOCR_WAVE], s_mx[TW / VOCR_WAVE];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int row_tiles = (h + ROWS - 1) / ROWS;
    const int ch = blockIdx.y / row_tiles, oy0 = (blockIdx.y - ch * row_tiles) * ROWS;
    const int oy_end = min(oy0 + ROWS, h);
    const int ox0 = blockIdx.x * TW, ox = ox0 + tid;
    const int w = min(max(widths[b], 0), wmax);
    const int nparts = gridDim.x * gridDim.y;
    float2* my_part = MINMAX ? part + (size_t)b * nparts + (size_t)blockIdx.y * gridDim.x + blockIdx.x : nullptr;
    float* yc = MINMAX ? nullptr : y + ((size_t)b * c + ch) * h * (size_t)wmax;

    if (ox0 >= w) {                                       // a tile of padding only (workgroup-uniform)
        if (MINMAX) {
            if (tid == 0) *my_part = make_float2(INFINITY, -INFINITY);
        } else if (ox < wmax) {
            for (int oy = oy0; oy < oy_end; ++oy) yc[(size_t)oy * wmax + ox] = 0.f;
        }
        return;
    }
    const bool have_mesh = mesh != nullptr && gw_max >= 1 && gh >= 1;
    const Line L = load_line(params + (size_t)b * REC, have_mesh, gw_max, with_filter);
    if (MINMAX && !L.filter) return;                      // nobody reads this line's partials
    const float* xc = x + ((size_t)b * c + ch) * h * (size_t)wmax;
    const int gws = gw_max + 1;
    const float* md = have_mesh ? mesh + (size_t)b * 2 * (gh + 1) * gws : nullptr;
    const float sx = (float)L.gw / (float)w, sy = (float)gh / (float)h;
    const bool live = ox < w;

    float mn = INFINITY, mx = -INFINITY;
    if (!MINMAX && L.filter) {                            // fold the line's partials: every wave for itself, no barrier
        for (int p = lane; p < nparts; p += VOCR_WAVE) {
            const float2 q = part[(size_t)b * nparts + p];
            mn = fminf(mn, q.x);
            mx = fmaxf(mx, q.y);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        }
    }
    const float den = mx - mn;

    float up_l = 0.f, up_c = 0.f;                         // R(oy - 1, ox - 1), R(oy - 1, ox); 0 above the line and left of it
    if (L.filter && live && oy0 > 0) {
        if (ox > 0) up_l = sample(xc, wmax, h, w, L, md, gh, gws, sx, sy, ox - 1, oy0 - 1);
        up_c = sample(xc, wmax, h, w, L, md, gh, gws, sx, sy, ox, oy0 - 1);
    }
    float lo = INFINITY, hi = -INFINITY;
    for (int oy = oy0; oy < oy_end; ++oy) {
        float v = 0.f;
        if (live) {
            const float r_c = sample(xc, wmax, h, w, L, md, gh, gws, sx, sy, ox, oy);
            v = r_c;
            if (L.filter) {
                const float r_l = ox > 0 ? sample(xc, wmax, h, w, L, md, gh, gws, sx, sy, ox - 1, oy) : 0.f;
                const float f = fmaf(L.k11, r_c, fmaf(L.k10, r_l, fmaf(L.k01, up_c, fmaf(L.k00, up_l, L.bias))));
                up_l = r_l;
                up_c = r_c;
                if (MINMAX) {
                    lo = fminf(lo, f);
                    hi = fmaxf(hi, f);
                } else {
                    v = den > 0.f ? (f - mn) / den : 0.f;
                }
            }
            if (!MINMAX) v = photometric(v, L, ch, oy, ox);
        }
        if (!MINMAX && ox < wmax) yc[(size_t)oy * wmax + ox] = v;
    }
    if (MINMAX) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if (lane == 0) {
            s_mn[tid >> 6] = lo;
            s_mx[tid >> 6] = hi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < TW / VOCR_WAVE; ++k) {
                lo = fminf(lo, s_mn[k]);
                hi = fmaxf(hi, s_mx[k]);
            }
            *my_part = make_float2(lo, hi);
        }
    }
}

bool shape_ok(int b, int c, int h, int wmax) {
    return b >= 1 && b <= 65535 && (c == 1 || c == 3) && h >= 1 && wmax >= 1 && h <= DIM_MAX && wmax <= DIM_MAX &&
           (long)c * vocr_cdiv(h, ROWS) <= 65535;
}

size_t parts_bytes(int b, int c, int h, int wmax) {
    return (size_t)b * c * vocr_cdiv(h, ROWS) * vocr_cdiv(wmax, TW) * sizeof(float2);
}

}  // namespace

extern "C" size_t vocr_augment_workspace_bytes(int b, int c, int h, int wmax) {
    return shape_ok(b, c, h, wmax) ? parts_bytes(b, c, h, wmax) : 0;
}

extern "C" int vocr_augment_lines(const float* x, const int32_t* widths, int b, int c, int h, int wmax, const uint32_t* params,
                                  const float* mesh, int gh, int gw_max, int with_filter, float* y, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* who = "vocr_augment_lines";
    VOCR_CHECK_ARG(b >= 1 && c >= 1 && h >= 1 && wmax >= 1, "%s: need b, c, h, wmax >= 1 (b=%d c=%d h=%d wmax=%d)", who, b, c, h, wmax);
    VOCR_CHECK_ARG(c == 1 || c == 3, "%s: c must be 1 or 3 (c=%d)", who, c);
    VOCR_CHECK_ARG(shape_ok(b, c, h, wmax), "%s: unsupported shape (b=%d c=%d h=%d wmax=%d): b <= 65535, h, wmax <= 2^24", who, b, c, h, wmax);
    VOCR_CHECK_ARG(x && widths && params && y, "%s: null pointer", who);
    const uintptr_t nb = (uintptr_t)b * c * h * wmax * sizeof(float), xa = (uintptr_t)x, ya = (uintptr_t)y;
    VOCR_CHECK_ARG(ya != xa && (ya + nb <= xa || xa + nb <= ya), "%s: y must not be x or overlap it (in place is refused)", who);
    VOCR_CHECK_ARG(mesh ? (gh >= 1 && gw_max >= 1 && gh <= DIM_MAX && gw_max < DIM_MAX) : true,
                   "%s: a mesh table needs gh >= 1 and gw_max >= 1 (gh=%d gw_max=%d)", who, gh, gw_max);
    const size_t need = parts_bytes(b, c, h, wmax);
    VOCR_CHECK_ARG(!with_filter || workspace, "%s: null pointer (the block filter needs the workspace)", who);
    VOCR_CHECK_ARG(!with_filter || workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    VOCR_CHECK_ARG(!with_filter || (((uintptr_t)workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(vocr_cdiv(wmax, TW), c * vocr_cdiv(h, ROWS), b);
    float2* part = with_filter ? (float2*)workspace : nullptr;
    if (with_filter) {
        augment_kernel<true><<<grid, TW, 0, s>>>(x, widths, c, h, wmax, params, mesh, gh, gw_max, 1, nullptr, part);
        VOCR_CHECK_LAUNCH("vocr_augment_lines(min/max)");
    }
    augment_kernel<false><<<grid, TW, 0, s>>>(x, widths, c, h, wmax, params, mesh, gh, gw_max, with_filter ? 1 : 0, y, part);
    VOCR_CHECK_LAUNCH("vocr_augment_lines(apply)");
    return VOCR_OK;
}
