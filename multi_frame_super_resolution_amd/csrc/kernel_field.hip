// kernel_field.hip -- the reference's kernel-shape field in one launch: E1 (5-point derivatives of the tracking image) +
// E2 (structure tensor) + the separable smoothing + E3 (ComputeKernelParam) + the float4 packing, for a row window of the
// field.  Bit-identical to the whole-image chain mfsr_ComputeDerivatives2Kernel -> mfsr_ComputeStructureTensor ->
// mfsr_separableFilter(chan = 3) -> mfsr_ComputeKernelParam -> mfsr_float3ToFloat4: every float operation comes from
// field_math.hpp / common.hpp, the functions the chain's kernels are built from, in the chain's order.
//
// Workgroup = KF_TX x KF_TY field pixels.  With h = ntaps / 2:
//   1. the tracking image under the tile, + h (smoothing halo) + KF_MARGIN (stencil reach) on every side, clipped to the image,
//      goes to LDS;
//   2. the bilinear coordinates of the stencil are separable: tex_coord's column half depends on the column alone, its row
//      half on the row alone.  They are evaluated once per tile column / row and stencil tap (5 each: +2, +1, -1, -2 steps
//      and the centre) with tex_coord itself and stored as LDS offsets + fraction.  An index outside the staged tile (no
//      image size is known to produce one; such workgroups are counted, mfsr_kernelParamFieldFallbacks, and the tests
//      require the count to stay zero) makes the workgroup take its derivatives from global memory with deriv5;
//   3. derivatives and tensor for the tile + h, where that is inside the image (the smoothing clamps at the image border);
//   4. smoothing along x for the tile's columns, rows + h; then along y, E3 and the store.
// Derivatives and tensor are recomputed on (TX + 2h)(TY + 2h) / (TX TY) of the pixels (1.33 at the default 5 taps) in
// exchange for five intermediates that never reach HBM.
#include <cstring>

#include "common.hpp"
#include "field_math.hpp"

#define KF_TX 64
#define KF_TY 16
#define KF_MAXH 5    // ntaps / 2 the kernel is built for (default_config: sigmaTensor 1 -> 5 taps, h = 2)
#define KF_MARGIN 3  // texels a bilinear fetch of the stencil reaches beyond its pixel: 2 steps + the interpolation partner
#define KF_THREADS 256

struct KfTaps {
    float t[2 * KF_MAXH + 1];
    int n;
};

struct KfParams {
    float Dth, Dtr, kDetail, kDenoise, kStretch, kShrink;
};

// one half of a TexCoord, as offsets into the staged image tile (columns: elements; rows: elements of whole tile rows)
struct KfCoord {
    int i0, i1;
    float a;
};

// i / d for i, d < 65536: magic = kf_magic(d), 0 standing for d == 1 (whose 2^32 / d does not fit)
__device__ __forceinline__ unsigned kf_magic(int d) { return d == 1 ? 0u : 0xffffffffu / (unsigned)d + 1u; }
__device__ __forceinline__ int kf_div(int i, unsigned magic) { return magic ? (int)__umulhi((unsigned)i, magic) : i; }

// workgroups that took their derivatives from global memory because a stencil index fell outside the staged tile (step 2 of
// the header): none is expected for any image size, and mfsr_kernelParamFieldFallbacks lets the tests hold the kernel to that
__device__ unsigned int g_kf_fallbacks;

__global__ void __launch_bounds__(KF_THREADS)
    k_kernelParamField(mfsr_tex2d tex, float4* __restrict__ out, int outPitch, int row0, int rowEnd, KfTaps taps, KfParams P)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int w = tex.width, H = tex.height;
    const int n = taps.n, h = n / 2;
    const int TWp = KF_TX + 2 * h, THp = KF_TY + 2 * h;            // tensor tile, at most
    const int IWp = TWp + 2 * KF_MARGIN, IHp = THp + 2 * KF_MARGIN;  // image tile, at most
    // the x-smoothed tensor takes the place of the image tile and the coordinate tables, which are dead by then
    const int imgFloats = IHp * IWp + 3 * 5 * (TWp + THp), xFloats = 3 * THp * KF_TX;
    float* s_T = s_mem;                               // [3][THp][TWp]
    float* s_img = s_T + 3 * THp * TWp;               // [IHp][IWp]
    KfCoord* s_cx = (KfCoord*)(s_img + IHp * IWp);    // [5][TWp]
    KfCoord* s_cy = s_cx + 5 * TWp;                   // [5][THp]
    float* s_X = s_img;                               // [3][THp][KF_TX]
    int* s_bad = (int*)(s_img + max(imgFloats, xFloats));
    const int tid = threadIdx.x;

    const int x0 = blockIdx.x * KF_TX, y0 = row0 + blockIdx.y * KF_TY;
    const int x1 = min(x0 + KF_TX, w), y1 = min(y0 + KF_TY, rowEnd);
    const int tx0 = max(x0 - h, 0), tx1 = min(x1 + h, w), ty0 = max(y0 - h, 0), ty1 = min(y1 + h, H);
    const int tw = tx1 - tx0, th = ty1 - ty0;
    const int ix0 = max(tx0 - KF_MARGIN, 0), ix1 = min(tx1 + KF_MARGIN, w);
    const int iy0 = max(ty0 - KF_MARGIN, 0), iy1 = min(ty1 + KF_MARGIN, H);
    const int iw = ix1 - ix0, ih = iy1 - iy0;
    const unsigned twMagic = kf_magic(tw), iwMagic = kf_magic(iw);

    if (tid == 0) *s_bad = 0;
    for (int i = tid; i < iw * ih; i += KF_THREADS) {
        const int r = kf_div(i, iwMagic), c = i - r * iw;
        s_img[r * IWp + c] = row_ptr((const float*)tex.ptr, tex.pitch, iy0 + r)[ix0 + c];
    }
    __syncthreads();  // (s_bad = 0 before the flags below)
    const float dx = 1.0f / (float)w;
    const float dy = 1.0f / (float)H;
    // tap k = 0..3: the stencil's steps along the axis; k = 4: the axis the stencil does not step along (d = 0)
    for (int i = tid; i < 5 * tw; i += KF_THREADS) {
        const int k = kf_div(i, twMagic), c = i - k * tw;
        const float x = ((float)(tx0 + c) + 0.5f) * dx;
        const float u = k < 4 ? deriv5_tap(x, dx, k) : deriv5_tap(x, 0.0f, 0);
        const TexCoord tc = tex_coord<ADDR_MIRROR>(w, H, u, 0.5f);
        if (tc.i0 < ix0 || tc.i0 >= ix1 || tc.i1 < ix0 || tc.i1 >= ix1) *s_bad = 1;
        KfCoord e = {tc.i0 - ix0, tc.i1 - ix0, tc.a};
        s_cx[k * TWp + c] = e;
    }
    const unsigned thMagic = kf_magic(th);
    for (int i = tid; i < 5 * th; i += KF_THREADS) {
        const int k = kf_div(i, thMagic), r = i - k * th;
        const float y = ((float)(ty0 + r) + 0.5f) * dy;
        const float v = k < 4 ? deriv5_tap(y, dy, k) : deriv5_tap(y, 0.0f, 0);
        const TexCoord tc = tex_coord<ADDR_MIRROR>(w, H, 0.5f, v);
        if (tc.j0 < iy0 || tc.j0 >= iy1 || tc.j1 < iy0 || tc.j1 >= iy1) *s_bad = 1;
        KfCoord e = {(tc.j0 - iy0) * IWp, (tc.j1 - iy0) * IWp, tc.b};
        s_cy[k * THp + r] = e;
    }
    __syncthreads();
    const bool staged = *s_bad == 0;  // uniform
    if (!staged && tid == 0) atomicAdd(&g_kf_fallbacks, 1u);

    // E1 + E2 on the tensor tile
    for (int i = tid; i < tw * th; i += KF_THREADS) {
        const int r = kf_div(i, twMagic), c = i - r * tw;
        float Ix, Iy;
        if (staged) {
            auto fetch = [&](const KfCoord& cx, const KfCoord& cy) {
                const float* r0 = s_img + cy.i0;
                const float* r1 = s_img + cy.i1;
                return lerp4(r0[cx.i0], r0[cx.i1], r1[cx.i0], r1[cx.i1], cx.a, cy.a);
            };
            const KfCoord xc = s_cx[4 * TWp + c], yc = s_cy[4 * THp + r];
            Ix = deriv5_of([&](int k) { return fetch(s_cx[k * TWp + c], yc); });
            Iy = deriv5_of([&](int k) { return fetch(xc, s_cy[k * THp + r]); });
        } else {
            const float x = ((float)(tx0 + c) + 0.5f) * dx;
            const float y = ((float)(ty0 + r) + 0.5f) * dy;
            Ix = deriv5(tex, x, y, dx, 0.0f);
            Iy = deriv5(tex, x, y, 0.0f, dy);
        }
        const pix3 t = tensor_products(Ix, Iy);
        s_T[r * TWp + c] = t.x;
        s_T[(THp + r) * TWp + c] = t.y;
        s_T[(2 * THp + r) * TWp + c] = t.z;
    }
    __syncthreads();

    // smoothing along x (k_filter1d<true>: columns clamped at the image border)
    const int c0 = n / 2;
    for (int i = tid; i < th * KF_TX; i += KF_THREADS) {
        const int r = i / KF_TX, c = i - r * KF_TX;
        const int x = x0 + c;
        if (x >= w) continue;
        for (int ch = 0; ch < 3; ch++) {
            const float* src = s_T + (ch * THp + r) * TWp;
            float s = 0;
            for (int t = 0; t < n; t++) s = filter_step(s, taps.t[t], src[clampi(x + t - c0, 0, w - 1) - tx0]);
            s_X[(ch * THp + r) * KF_TX + c] = s;
        }
    }
    __syncthreads();

    // smoothing along y (k_filter1d<false>: rows clamped at the image border), E3, float4
    for (int i = tid; i < (y1 - y0) * KF_TX; i += KF_THREADS) {
        const int r = i / KF_TX, c = i - r * KF_TX;
        const int x = x0 + c, y = y0 + r;
        if (x >= w) continue;
        float g[3];
        for (int ch = 0; ch < 3; ch++) {
            const float* src = s_X + ch * THp * KF_TX + c;
            float s = 0;
            for (int t = 0; t < n; t++) s = filter_step(s, taps.t[t], src[(clampi(y + t - c0, 0, H - 1) - ty0) * KF_TX]);
            g[ch] = s;
        }
        const pix3 grad = {g[0], g[1], g[2]};
        const pix3 p = kernel_param(grad, P.Dth, P.Dtr, P.kDetail, P.kDenoise, P.kStretch, P.kShrink);
        row_ptr(out, outPitch, y)[x] = make_float4(p.x, p.y, p.z, 0.0f);
    }
}

static size_t kf_lds_bytes(int h)
{
    const size_t TWp = KF_TX + 2 * h, THp = KF_TY + 2 * h, IWp = TWp + 2 * KF_MARGIN, IHp = THp + 2 * KF_MARGIN;
    const size_t imgFloats = IHp * IWp + 3 * 5 * (TWp + THp), xFloats = 3 * THp * KF_TX;
    static_assert(sizeof(KfCoord) == 3 * sizeof(float), "the coordinate tables are counted in floats");
    return sizeof(float) * (3 * THp * TWp + (imgFloats > xFloats ? imgFloats : xFloats)) + sizeof(int);
}

// 1 (default): set_reference takes the fused reference setup (this file, mfsr_tileSquaredSumsLevels, mfsr_deBayerFusedRing);
// 0: the kernel chain
static std::atomic<int> g_reference_fused{1};
extern "C" int mfsr_set_reference_fused(int enable)
{
    g_reference_fused = enable ? 1 : 0;
    return MFSR_OK;
}
int mfsr_reference_fused() { return g_reference_fused; }

extern "C" int mfsr_kernelParamField(mfsr_tex2d tex, mfsr_tex2d field, int row0, int rows, const float* taps, int ntaps, float Dth,
                                     float Dtr, float kDetail, float kDenoise, float kStretch, float kShrink, mfsr_stream_t stream)
{
    MFSR_REQUIRE(taps && ntaps > 0 && ntaps <= 99);
    MFSR_REQUIRE(mfsr_tex_ok(tex, 4) && (tex.pitch & 3) == 0 && ((uintptr_t)tex.ptr & 3) == 0);
    MFSR_REQUIRE(mfsr_tex_ok(field, 16) && (field.pitch & 15) == 0 && ((uintptr_t)field.ptr & 15) == 0);
    MFSR_REQUIRE(field.width == tex.width && field.height == tex.height);
    MFSR_REQUIRE(row0 >= 0 && rows > 0 && row0 + rows <= tex.height);
    if (ntaps / 2 > KF_MAXH || tex.width < KF_TX || tex.height < KF_TY) return MFSR_E_UNSUPPORTED;
    KfTaps tp;
    memset(&tp, 0, sizeof(tp));
    memcpy(tp.t, taps, sizeof(float) * ntaps);
    tp.n = ntaps;
    const KfParams P = {Dth, Dtr, kDetail, kDenoise, kStretch, kShrink};
    dim3 grid(mfsr_cdiv(tex.width, KF_TX), mfsr_cdiv(rows, KF_TY));
    hipLaunchKernelGGL(k_kernelParamField, grid, dim3(KF_THREADS), kf_lds_bytes(ntaps / 2), mfsr_s(stream), tex, (float4*)field.ptr,
                       field.pitch, row0, row0 + rows, tp, P);
    return mfsr_launch_status("kernelParamField");
}

// workgroups of all mfsr_kernelParamField launches so far (since the last reset) that left the staged path; synchronises
extern "C" int mfsr_kernelParamFieldFallbacks(int* count, int reset)
{
    MFSR_REQUIRE(count != nullptr);
    unsigned int n = 0;
    MFSR_HIP_TRY(hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_kf_fallbacks), sizeof(n)));
    *count = (int)n;
    if (reset) {
        n = 0;
        MFSR_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_kf_fallbacks), &n, sizeof(n)));
    }
    return MFSR_OK;
}
