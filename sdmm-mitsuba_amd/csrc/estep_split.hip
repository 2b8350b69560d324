// estep_split.hip -- responsibility E-step with the eight linear forms on the
// bf16 matrix cores, exact to fp32 by a three-way bf16 split of both operands.
//
// Replaces the N x K loop of MixtureModel::posteriorAndLog
// (mitsuba/src/integrators/dmm/jmm/mixture_model.h:146-192) over
// MultivariateTangentNormal::pdfAndLog / TangentSpace::log
// (multivariate_tangent_normal.h:146-177, :350-365), like estep_resp_tile_kernel
// (estep.hip) and with the same pair formula; only the linear forms move.
//
// Per (sample n, component k) the pdf needs eight LINEAR forms of the sample
// (estep_mfma.hip header): c = R2.d, ad = (L33 R0).d, bd = (L43 R0 + L44 R1).d,
// and u_m = sum_j L_mj (p_j - o) + NC_m, m = 0..4 (o = kOrigin, NC_m = EP_NC*).
// In the VALU tile kernel they are 21 of the 42 packed FMAs per pair.  Here
// they are v_mfma_f32_16x16x32_bf16 products D[16 samples][16 components] =
// A[16][32] . B[32][16], one MFMA per form and 16 x 16 block:
//
//   * every fp32 operand x is split exactly into three bf16 x = h + m + l
//     (round-to-nearest h, then m of the exact remainder x - h, then l of the
//     exact remainder, which has at most 8 significant bits left);
//   * a product c x is the six largest of the nine split products,
//     hc.h + mc.h + hc.m + lc.h + hc.l + mc.m, each exact in the fp32
//     accumulator; the three dropped ones are below 2^-25 |c x| together (half
//     an fp32 ulp), so every form carries fp32-level error like the FMA chain
//     it replaces (the responsibility bound of tests/test_gpu_parity.py
//     _check_resp holds, as for the f32 MFMA kernel);
//   * the K = 32 reduction of one MFMA holds one feature per 8-lane k group:
//     lane group g = lane >> 4 (g < 3) owns feature g, its eight k entries
//     pair A = [h h m h l m e6 e7] of the sample with B = [hc mc hc lc hc mc
//     X6 X7] of the coefficient; the spatial forms put their constant NC_m in
//     e6/e7 = 1 and X6/X7 = NC's split (group 0: h, m; group 1: l), group 3 is
//     zero.  Building one A fragment is 7 VALU per 16 samples;
//   * the rows of u (spatial forms, ad, bd) carry the factor sqrt(log2(e)/2)
//     (fp64 product rounded to fp32 before the split), so the exponent of
//     NORM5 exp(-q/2) is one FMA chain (pdf_pair).
//
// The B image of the whole mixture (R = Kp/16 blocks x 8 forms x 64 lanes x 16
// B = R x 8 KB, 64 KB at K = 128) is built once per parameter change by
// estep_resp_image_kernel into a global buffer of the handle, copied into LDS
// by each workgroup and read as one ds_read_b128 per fragment, conflict-free
// (SDMM_RESP_IMAGE=inline: every workgroup builds it from the E-step record
// itself, as before the image was cached; the same bits either way).  The
// D layout gives each lane one component (col = lane & 15) of four samples
// (rows 4 (lane >> 4) + j); the nonlinear rest of the pair math (angle, exp,
// pdf) runs packed over sample pairs (j, j+1), the posterior normaliser sums
// the lane's own 4 R components and then the sample's four lane groups by two
// row swaps (v_permlane16_swap, v_permlane32_swap), and the rows go out as
// 16-B stores (K = 128: staged through LDS into 256-B half rows).
//
// At R = 8 the default is the band form further down (resp_band_body): the
// image stays in registers, a wave owning 32 components instead of 16 samples.
#include "sdmm_device.h"
#include "launch.h"

namespace sdmm {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

template <bool B> struct Tag { static constexpr bool value = B; };

constexpr float kLog2Norm5S = -6.628740082514092f;   // log2((float)pow(0.39894228f, 5)), mvtn.h:351-352

__device__ __forceinline__ f2 spl(float x) { return (f2)(x); }
__device__ __forceinline__ f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 pmul(f2 a, f2 b) { return a * b; }
__device__ __forceinline__ f2 padd(f2 a, f2 b) { return a + b; }

// two floats -> one dword of two bf16 (round to nearest even): element 0 (lo)
// in bits 0..15, element 1 (hi) in bits 16..31 (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pk(float lo, float hi) {
    const bf2 v = __builtin_convertvector(f2{lo, hi}, bf2);
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float hi_of(unsigned d) { return __builtin_bit_cast(float, d & 0xFFFF0000u); }
__device__ __forceinline__ float lo_of(unsigned d) { return __builtin_bit_cast(float, d << 16); }

// Split x into (h, m, l) bf16 parts as floats' dwords: see the header.
// Sample fragment of one lane (K layout in the header): lane group g < 3 holds
// the small products of feature g, [h m h l m e5 e6 0]; group 3 holds the
// three large ones and the constant's largest part, [0 0 0 0 x0h x1h x2h e7].
// x: the sample's three features; spatial: the forms with the constant NC.
__device__ __forceinline__ bf8 a_frag(const float (&x)[3], int g, bool spatial) {
    const float xg = g == 0 ? x[0] : (g == 1 ? x[1] : x[2]);   // (g < 3)
    const unsigned t = pk(xg, xg);
    const float r1 = xg - hi_of(t);               // exact
    const unsigned d0 = pk(xg, r1);               // (h, m)
    const float r2 = r1 - hi_of(d0);              // exact, <= 8 significant bits
    const unsigned d1 = pk(xg, r2);               // (h, l)
    const bool cst = spatial && g == 0;
    const unsigned d2 = pk(r1, cst ? 1.0f : 0.0f);   // (m, e5)
    const unsigned d3 = cst ? 0x3F80u : 0u;          // (e6, 0)
    const unsigned q2 = pk(x[0], x[1]);              // (x0h, x1h)
    const unsigned q3 = pk(x[2], spatial ? 1.0f : 0.0f);   // (x2h, e7)
    return __builtin_bit_cast(bf8, g < 3 ? u4{d0, d1, d2, d3} : u4{0u, 0u, q2, q3});
}

// (h, m, l) of an fp32 value as bf16 bit patterns
__device__ __forceinline__ void split3(float c, unsigned& h, unsigned& m, unsigned& l) {
    const unsigned hh = pk(c, c);
    const float r1 = c - hi_of(hh);
    const unsigned mm = pk(r1, r1);
    const float r2 = r1 - lo_of(mm);
    const unsigned ll = pk(r2, r2);
    h = hh & 0xFFFFu;
    m = mm & 0xFFFFu;
    l = ll & 0xFFFFu;
}

// sqrt(log2(e) / 2): the rows of u (spatial forms, ad, bd) are pre-scaled by
// it, so that the exponent 2^(log2 NORM5 - |u'|^2) = NORM5 exp(-q/2) is one
// FMA chain from the constant (no separate q and scaling step)
constexpr bool kFoldScale = true;
constexpr double kRowScale = 0.84932180028801904272;

// row start of L^-1 row m in the packed lower triangle (EP_L00 ...)
__device__ __forceinline__ int lrow(int m) { return EP_L00 + m * (m + 1) / 2; }

// Coefficient fragment of block r, form f, lane l (the A operand of the
// MFMA; K layout in the header): lane group g < 3 pairs feature g's small
// products, [cm ch cl ch cm X5 X6 0] with X5, X6 = NC's l, m parts in group 0
// of the spatial forms; group 3 holds [0 0 0 0 c0h c1h c2h X7], X7 = NC's h
// part.  Forms: 0 c (R2), 1 ad (A), 2 bd (B), 3 + m the spatial row m
// (L_m0..L_m2 of L^-1, constant NC_m(o) = -sum_j L_mj (mu_j - o) in fp64).
__device__ __forceinline__ u4 coef_frag(const float* __restrict__ ep, int Kp, int r, int f, int l,
                                        const float* __restrict__ o) {
    const int k = 16 * r + (l & 15);
    const int g = l >> 4;
    float c[3];
    unsigned nh = 0u, nm = 0u, nl = 0u;
    if (f < 3) {
        const int base = f == 0 ? EP_R20 : (f == 1 ? EP_A0 : EP_B0);
        for (int j = 0; j < 3; ++j) {
            c[j] = ep[(base + j) * Kp + k];
            if (f > 0) c[j] = (float)((double)c[j] * kRowScale);
        }
    } else {
        const int m = f - 3;
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) {
            const bool z = m <= 2 && j > m;
            c[j] = z ? 0.0f : (float)((double)ep[(lrow(m) + j) * Kp + k] * kRowScale);
            if (!z) acc += (double)ep[(lrow(m) + j) * Kp + k] * ((double)ep[(EP_MU0 + j) * Kp + k] - (double)o[j]);
        }
        split3((float)(-acc * kRowScale), nh, nm, nl);
    }
    if (g < 3) {
        unsigned h, m, lo;
        split3(c[g], h, m, lo);
        const unsigned x5 = g == 0 ? nl : 0u, x6 = g == 0 ? nm : 0u;
        return u4{m | (h << 16), lo | (h << 16), m | (x5 << 16), x6};
    }
    unsigned h0, h1, h2, t1, t2;
    split3(c[0], h0, t1, t2);
    split3(c[1], h1, t1, t2);
    split3(c[2], h2, t1, t2);
    return u4{0u, 0u, h0 | (h1 << 16), h2 | (nh << 16)};
}

// x + (x of lane ^ 16), then + (that of lane ^ 32): the sum over the four
// 16-lane rows, in every lane.  The swaps exchange the odd rows (the upper
// half) of one copy with the even rows (the lower half) of the other, so the
// two results are the lane's own value and its partner's in one VALU each (no
// LDS crossbar, no lane-index arithmetic, no lgkmcnt wait); builtins, so the
// compiler places the VALU-write hazard waits.
__device__ __forceinline__ float rows_sum4(float x) {
    const unsigned b = __builtin_bit_cast(unsigned, x);
    const auto p = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    const float y = __builtin_bit_cast(float, (unsigned)p[0]) + __builtin_bit_cast(float, (unsigned)p[1]);
    const unsigned c = __builtin_bit_cast(unsigned, y);
    const auto q = __builtin_amdgcn_permlane32_swap(c, c, false, false);
    return __builtin_bit_cast(float, (unsigned)q[0]) + __builtin_bit_cast(float, (unsigned)q[1]);
}

// pi_k pdf_k of the four (sample, component) pairs of one D fragment, as two
// packed pairs (rows j, j+1) advanced in lockstep (two independent chains per
// step: no dependency wait states between the packed FMAs), from the eight
// row-scaled forms u' = sqrt(log2(e)/2) u, so NORM5 exp(-q/2) =
// 2^(log2 NORM5 - |u'|^2) (estep.hip pair_q_tile).  The angle is
// estep.hip angle_over_sin_main's (degree-7 h(u), pi/sqrt(1-c^2) - h(u) for
// c < 0); RARE adds the reference's quirks (mvtn.h:157-164) for the far side:
// a = 1 where sin < 1e-3, a = 0 (failed log map) at c <= -1.
template <bool RARE>
__device__ __forceinline__ void pdf_quad(const f4& C, const f4& AD, const f4& BD, const f4& U0, const f4& U1,
                                         const f4& U2, const f4& S3, const f4& S4, const f4& dipi, f2 (&p)[2]) {
    f2 c[2], s2[2], u[2], h[2], a[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) c[i] = f2{C[2 * i], C[2 * i + 1]};
#pragma unroll
    for (int i = 0; i < 2; ++i) s2[i] = pfma(-c[i], c[i], spl(1.0f));
    // u = (1 - |c|)/2 as VOP3 FMAs with the |.| source modifier (packed FMAs
    // have none; this file is built with -fno-slp-vectorize so the compiler
    // does not re-pack them as v_and + v_pk_fma).  Not inline asm: the
    // compiler's MFMA-result hazard waits do not cover asm operands.
#pragma unroll
    for (int i = 0; i < 2; ++i) u[i] = f2{fmaf(-0.5f, fabsf(c[i].x), 0.5f), fmaf(-0.5f, fabsf(c[i].y), 0.5f)};
    constexpr float kH[8] = {3.3755881786346436f, -3.17423415184021f, 2.1241207122802734f, -0.04515757039189339f,
                             0.5178175568580627f, 0.5294308066368103f, 0.6667603850364685f, 0.9999996423721313f};
#pragma unroll
    for (int i = 0; i < 2; ++i) h[i] = pfma(spl(kH[0]), u[i], spl(kH[1]));
#pragma unroll
    for (int t = 2; t < 8; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i) h[i] = pfma(h[i], u[i], spl(kH[t]));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f2 r = f2{__builtin_amdgcn_rsqf(s2[i].x), __builtin_amdgcn_rsqf(s2[i].y)};
        const f2 fneg = pfma(spl(3.14159265358979f), r, -h[i]);
        if constexpr (!RARE) {
            // c < 0 ? fneg : h as one median: fneg > h on both sides (pi / s >
            // 2 acos|c| / s), and -2^100 c is +huge for c < 0 and -huge for
            // c > 0, so med3(h, fneg, -2^100 c) picks fneg or h (one packed
            // product + one med3 per pair instead of a compare + a select).
            // Only |c| < 2^-90 lands between (the result then h within
            // ~1e-7: pi / s - 2 h ~ 0 there), NaN pairs go to the RARE redo.
            const f2 t = pmul(c[i], spl(-0x1p100f));
            a[i] = f2{__builtin_amdgcn_fmed3f(h[i].x, fneg.x, t.x), __builtin_amdgcn_fmed3f(h[i].y, fneg.y, t.y)};
        } else {
            a[i] = f2{c[i].x < 0.0f ? fneg.x : h[i].x, c[i].y < 0.0f ? fneg.y : h[i].y};
        }
        if constexpr (RARE) {
            const float o0 = __builtin_amdgcn_fmed3f(1073741824.0f * (c[i].x + 1.0f), 0.0f, 1.0f);
            const float o1 = __builtin_amdgcn_fmed3f(1073741824.0f * (c[i].y + 1.0f), 0.0f, 1.0f);
            a[i].x = (c[i].x < 0.0f && s2[i].x < 1e-6f) ? o0 : a[i].x;
            a[i].y = (c[i].y < 0.0f && s2[i].y < 1e-6f) ? o1 : a[i].y;
        }
    }
    // detInv pi_k * jacobian (mvtn.h:361, mixture_model.h:164) ahead of the
    // exponent chain: the tail after the exp is one product per pair
    f2 da[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) da[i] = pmul(f2{dipi[2 * i], dipi[2 * i + 1]}, a[i]);
    f2 arg[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f2 u0 = f2{U0[2 * i], U0[2 * i + 1]};
        arg[i] = kFoldScale ? pfma(-u0, u0, spl(kLog2Norm5S)) : pmul(u0, u0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f2 u1 = f2{U1[2 * i], U1[2 * i + 1]};
        arg[i] = kFoldScale ? pfma(-u1, u1, arg[i]) : pfma(u1, u1, arg[i]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f2 u2 = f2{U2[2 * i], U2[2 * i + 1]};
        arg[i] = kFoldScale ? pfma(-u2, u2, arg[i]) : pfma(u2, u2, arg[i]);
    }
    f2 u3[2], u4[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        u3[i] = pfma(a[i], f2{AD[2 * i], AD[2 * i + 1]}, f2{S3[2 * i], S3[2 * i + 1]});
        u4[i] = pfma(a[i], f2{BD[2 * i], BD[2 * i + 1]}, f2{S4[2 * i], S4[2 * i + 1]});
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) arg[i] = kFoldScale ? pfma(-u3[i], u3[i], arg[i]) : pfma(u3[i], u3[i], arg[i]);
#pragma unroll
    for (int i = 0; i < 2; ++i) arg[i] = kFoldScale ? pfma(-u4[i], u4[i], arg[i]) : pfma(u4[i], u4[i], arg[i]);
    if constexpr (!kFoldScale) {
#pragma unroll
        for (int i = 0; i < 2; ++i) arg[i] = pfma(arg[i], spl(-0.72134752044448170368f), spl(kLog2Norm5S));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f2 e = f2{__builtin_amdgcn_exp2f(arg[i].x), __builtin_amdgcn_exp2f(arg[i].y)};
        p[i] = pmul(e, da[i]);
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Sample features through LDS by DMA, with counted waits (round 5).
//
// vmcnt counts loads and stores together, in issue order, and the compiler
// waits vmcnt(0) before the first use of a VGPR load whenever stores are
// pending beside it.  With the features loaded into VGPRs every tile, each
// wave therefore waited for ALL of its row stores before it could start the
// next tile: compute and the write stream took turns instead of overlapping
// (store-only shape 135 us against the 88-105 us write stream, the math then
// +45 us on top).  Here the features of tile t + kFeatAhead go by
// global_load_lds_dword (inline asm: the compiler does not track them, so it
// never drains vmcnt for them) into a per-wave LDS ring, and the wave waits
// with an explicit vmcnt(N) that leaves every store younger than that DMA in
// flight: N = 2 kFeatAhead + R k, the two DMA pieces of each tile issued after
// it plus the R row stores of each of the k = min(i, kFeatAhead + 1) flushes
// issued after it (every one of them a full flush of exactly R stores; any
// other flush in that window and the wait is vmcnt(0)).
constexpr int kFeatAhead = 2;
constexpr int kFeatSlots = kFeatAhead + 1;
constexpr int kFeatSlotU4 = 32;   // two 256-B DMA pieces (64 lanes x 4 B)

// vmcnt(N), then this lane's two 16-B feature records from the ring, in ONE
// statement: the compiler sees neither the DMA that wrote the ring nor its
// wait, so a plain read of the ring would be a read of memory it believes
// unwritten (undef: it did fold one of them to an unrelated register).
// lgkmcnt(0) inside: the outputs are complete when the statement ends.
template <int N>
__device__ __forceinline__ void read_feat(unsigned addr, f4& a, f4& b) {
    static_assert(N >= 0 && N <= 63, "gfx950 vmcnt is six bits");
    asm volatile(
        "s_waitcnt vmcnt(%3)\n\t"
        "ds_read_b128 %0, %2\n\t"
        "ds_read_b128 %1, %2 offset:256\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(a), "=&v"(b)
        : "v"(addr), "n"(N)
        : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N <= 63, "gfx950 vmcnt is six bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// (diagnostic SDMM_SPLIT_DIAG_NOSTORE: every row computed, none stored -- the
// compute-only time of the kernel; then only the DMAs are in flight)
#ifdef SDMM_SPLIT_DIAG_NOSTORE
constexpr bool kDiagNoStore = true;
#else
constexpr bool kDiagNoStore = false;
#endif
template <int R>
__device__ __forceinline__ void read_feat_counted(int k, bool window_full, unsigned addr, f4& a, f4& b) {
    if (kDiagNoStore) {
        read_feat<2 * kFeatAhead>(addr, a, b);
        return;
    }
    if (!window_full) {
        read_feat<0>(addr, a, b);
        return;
    }
    switch (k) {   // wave-uniform
        case 0: read_feat<2 * kFeatAhead>(addr, a, b); break;
        case 1: read_feat<2 * kFeatAhead + R>(addr, a, b); break;
        case 2: read_feat<2 * kFeatAhead + 2 * R>(addr, a, b); break;
        default: read_feat<2 * kFeatAhead + 3 * R>(addr, a, b); break;
    }
    static_assert(kFeatAhead == 2, "read_feat_counted enumerates k = 0 .. kFeatAhead + 1");
}

// two LDS-DMA pieces: lane L's dword of a0 to lds[L], of a1 to lds[64 + L]
// (M0 = the wave-uniform LDS byte address of the piece)
__device__ __forceinline__ void dma_pair(uintptr_t a0, uintptr_t a1, unsigned lds0) {
    unsigned keep;   // M0 is reserved by the compiler: saved and restored around the pieces
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %1, off\n\t"
        "s_mov_b32 m0, %4\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %2, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(a0), "v"(a1), "s"(lds0), "s"(lds0 + 256u)
        : "memory");
}

// The coefficient image in the order of the LDS carve: the R * 8 * 64
// fragments at (r * 8 + f) * 64 + lane, then the R * 4 detInv pi quads
// (components 16 r + 4 g .. + 3 at r * 4 + g).  One thread per 16-B entry.
__device__ __forceinline__ u4 image_entry(const float* __restrict__ ep, int Kp, int idx, int nc) {
    const float o_scene[3] = {kOrigin, kOrigin, kOrigin};
    if (idx < nc) return coef_frag(ep, Kp, idx >> 9, (idx >> 6) & 7, idx & 63, o_scene);
    const float* d = ep + EP_DIPI * Kp + 4 * (idx - nc);
    return __builtin_bit_cast(u4, f4{d[0], d[1], d[2], d[3]});
}

__global__ void __launch_bounds__(256) estep_resp_image_kernel(const float* __restrict__ ep, int Kp,
                                                               u4* __restrict__ img) {
    const int R = Kp / 16, nc = R * 8 * 64, nd = R * 4;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < nc + nd) img[idx] = image_entry(ep, Kp, idx, nc);
}

// INLINE: the workgroup builds the image from ep (img unused); otherwise it
// copies the prebuilt image img (estep_resp_image_kernel's, of this ep).
template <int R, int WPB, bool INLINE>
__device__ __forceinline__ void resp_split_body(const float* __restrict__ ep, const u4* __restrict__ img, int Kp, int K,
                                                const SamplesDev& s, int64_t n, int64_t nwaves,
                                                float* __restrict__ resp) {
    // one LDS block carved into: per wave the feature ring (kFeatSlots x 512 B;
    // first, so every LDS-DMA destination lies below 64 KB), the coefficient
    // image (R blocks x 8 forms x 64 lanes), detInv pi of components 16 r + 4 g
    // .. + 3 (the D rows of lane group g), and per wave the 256-B half-row
    // stage (R = 8: 16 rows)
    constexpr int NC = R * 8 * 64, ND = R * 4, NS = R == 8 ? 16 * 16 : 0, NF = kFeatSlots * kFeatSlotU4;
    constexpr int NTOT = WPB * NF + NC + ND + WPB * NS;
    static_assert(NTOT * 16 <= 163840, "the carved LDS block exceeds the 160 KB of a CU");
    static_assert(WPB * NF * 16 <= 65536, "LDS-DMA destinations stay below 64 KB");
    __shared__ u4 smem[NTOT];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    u4* const ring = smem + wid * NF;
    u4* const cimg = smem + WPB * NF;
    f4* const dimg = (f4*)(cimg + NC);
    f4* const st = (f4*)(cimg + NC + ND + wid * NS);
    static_assert(WPB * NF + NC + ND + WPB * NS == NTOT && (R != 8 || NS == 256), "LDS carve: every region has storage");

    // cimg and dimg are one run of NC + ND entries, in the image's order
    if constexpr (INLINE) {
        for (int idx = threadIdx.x; idx < NC + ND; idx += 64 * WPB) cimg[idx] = image_entry(ep, Kp, idx, NC);
    } else {
        // a straight copy: all of the thread's 16-B loads issued, then its LDS
        // writes (the last trip is partial: its load is clamped, its write is not done)
        constexpr int T = 64 * WPB, TRIPS = (NC + ND + T - 1) / T;
        u4 v[TRIPS];
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int idx = (int)threadIdx.x + i * T;
            v[i] = img[idx < NC + ND ? idx : NC + ND - 1];
        }
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int idx = (int)threadIdx.x + i * T;
            if (idx < NC + ND) cimg[idx] = v[i];
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    // the launch's 16-sample tiles dealt round robin over its waves (one round
    // of resident waves: each workgroup fills its coefficient image once):
    // wave w serves tiles w, w + nwaves, ..., so the waves running at one time
    // write neighbouring 8-KB row blocks.  (A contiguous range per wave put the
    // 2048 waves' concurrent rows 256 KB apart -- the same HBM channel bits --
    // and one configuration ran 170-190 or 340-370 us per launch depending on
    // where the output buffer landed.)
    // Waves are numbered in quads across the workgroups (nwaves = WPB gridDim):
    // waves 4 q .. 4 q + 3 of a workgroup, one per SIMD, take four neighbouring
    // tiles, and quad q of workgroup b comes before quad q + 1 of any.  The
    // T mod nwaves waves that serve one tile more are then the first quads of
    // EVERY workgroup, evenly over the SIMDs, and not all WPB waves of the
    // first workgroups (block WPB + wid gave 85 CUs 66 tiles per SIMD and the
    // rest 63 at N = 2^20; now 64 everywhere).  A quad and not single waves
    // (wid gridDim + block): a tile reads 64 B of each fp32 plane and 16 B of
    // the flag bytes, and with neighbouring tiles on different workgroups
    // (other XCDs' L2s) every 128-B line was fetched twice, the flags' eight
    // times: 67.6 against 31.2 MB read per launch at N = 2^20 (FETCH_SIZE).
    static_assert(WPB % 4 == 0, "the deal numbers a workgroup's waves in quads");
    const int64_t wave = 4 * ((int64_t)(wid >> 2) * gridDim.x + blockIdx.x) + (wid & 3);
    const int64_t s0 = 16 * wave, step = 16 * nwaves, s1 = n;
    if (wave >= nwaves || s0 >= n) return;
    // The wave's run in 32-bit counts (SALU compares; there is no 64-bit
    // scalar order compare): jfull tiles of 16 rows, then at most one that
    // crosses s1 with rows_last rows (the next one lies wholly past the end:
    // step >= 16), nit tiles in all.
    const uint64_t span = (uint64_t)(s1 - s0), whole = span - 16;
    const int jfull = span < 16          ? 0
                      : (whole >> 32) == 0 ? (int)((uint32_t)whole / (uint32_t)step) + 1
                                           : (int)(whole / (uint64_t)step) + 1;
    const int64_t tl = s0 + jfull * step;   // the first tile that is not whole
    const int rows_last = tl < s1 ? (int)(s1 - tl) : 0;
    const int nit = jfull + (rows_last > 0 ? 1 : 0);

    // MFMA D[component][sample] = A[component][k] . B[k][sample]: A = the
    // coefficient fragment (lane: component 16 r + (lane & 15), k group
    // lane >> 4), B = the sample fragment (lane: feature g of sample col);
    // D gives lane (g, col) components 16 r + 4 g + j (j = 0..3) of sample col
    const int g = lane >> 4;
    const int col = lane & 15;
    const bool has_h = s.hpdf != nullptr, has_d = s.isDiffuse != nullptr;

    // DMA sources of this lane: sample sl = lane >> 2 of the tile, plane pl =
    // lane & 3 of piece 0 (x0 x1 x2 x3) and of piece 1 (x4 x5 hpdf isDiffuse;
    // an absent optional plane re-reads x0).  The diffuse flag comes as the
    // dword that holds its byte (the plane's dword-aligned word).
    const int pl = lane & 3, sl = lane >> 2;
    const uintptr_t src0 = (uintptr_t)(pl == 0 ? s.x[0] : pl == 1 ? s.x[1] : pl == 2 ? s.x[2] : s.x[3]);
    const bool byteplane = pl == 3 && has_d;
    const uintptr_t src1 = (uintptr_t)(pl == 0   ? s.x[4]
                                       : pl == 1 ? s.x[5]
                                       : pl == 2 ? (has_h ? s.hpdf : s.x[0])
                                                 : (has_d ? (const float*)s.isDiffuse : s.x[0]));
    const int sh1 = byteplane ? 0 : 2;
    const unsigned ring_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) u4*)ring;
    // The lane's two source addresses run with the tiles: dma() is called for
    // the wave's tiles 0, 1, ... in order and advances them by the step (32
    // bits: the launcher bounds nwaves), the byte plane's in bytes.  A tile
    // that is not whole (wave-uniform: the end of the wave's run) reads the
    // clamped samples of tile jfull instead -- past the end any valid sample
    // does, those records are never used -- and the branch is kept a branch
    // (the empty asm: not four selects on every tile).
    uintptr_t dp0 = src0 + ((uintptr_t)(s0 + sl) << 2);
    uintptr_t dp1 = src1 + ((uintptr_t)(s0 + sl) << sh1);
    const unsigned dstep0 = (unsigned)step << 2, dstep1 = (unsigned)step << sh1;
    const int64_t il = tl + sl < s1 ? tl + sl : s1 - 1;
    const uintptr_t last0 = src0 + ((uintptr_t)il << 2), last1 = src1 + ((uintptr_t)il << sh1);
    auto dma = [&](int j, int slot) __attribute__((always_inline)) {
        if (j >= jfull) {
            asm volatile("");
            dp0 = last0;
            dp1 = last1;
        }
        dma_pair(dp0, dp1 & ~(uintptr_t)3, ring_lds + (unsigned)slot * (kFeatSlotU4 * 16u));
        dp0 += dstep0;
        dp1 += dstep1;
    };

    auto pfrag = [&](const float (&p3)[3]) __attribute__((always_inline)) {
        const float x[3] = {p3[0] - kOrigin, p3[1] - kOrigin, p3[2] - kOrigin};
        return a_frag(x, g, true);
    };
    // block r's coefficient fragments and detInv pi of the lane's four components
    auto frags = [&](int r, bf8 (&F)[8], f4& dp) __attribute__((always_inline)) {
#pragma unroll
        for (int f = 0; f < 8; ++f) F[f] = __builtin_bit_cast(bf8, cimg[(r * 8 + f) * 64 + lane]);
        dp = dimg[r * 4 + g];
    };
    auto forms = [&](const bf8 (&F)[8], bf8 bs, bf8 bd, f4 (&D)[8]) __attribute__((always_inline)) {
        const f4 z = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int f = 0; f < 8; ++f) D[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[f], f < 3 ? bd : bs, z, 0, 0, 0);
    };

    // The rows of tile t are stored at the top of the next tile (flush), after
    // the DMA of the features kFeatAhead tiles ahead; a full flush is exactly
    // R store instructions (the count read_feat_counted relies on).
    // Row addresses: the tile's first row is a wave-uniform 64-bit base (SGPRs,
    // advanced by the step's rows each tile) and the lane adds a 32-bit byte
    // offset inside the tile, fixed before the loop (at most 16 rows of K
    // floats: small for any n, nothing here is a product with a row index).
    // A full tile has K = 16 R, so its offsets are constants of the lane.
    float pdf[R][4];
    float gsc_p = 0.0f;
    bool full_p = false;
    char* rowp = nullptr;   // the pending tile's first row (none yet)
    int rows_p = 0;         // ... and its rows below s1 (16 unless it crosses s1)
    char* rowt = (char*)(resp + s0 * (int64_t)K);
    const int64_t rowstep = step * (int64_t)K * 4;
    const unsigned voff = (unsigned)(col * K + 4 * g) * 4u;                     // row col, block 0's 16 B
    const unsigned voff8 = (unsigned)(g * (16 * R) + 4 * col) * 4u;             // R = 8: row g, 16-B chunk col
    auto flush = [&]() __attribute__((always_inline)) {
        if (rowp == nullptr) return;
        if (kDiagNoStore && gsc_p != -1.0f) return;   // (never -1: the rows stay live)
        if (full_p && R != 8) {
            // one 16-B store per block: a sample's 64-B row segment per 4 lanes
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const f2 lo = f2{pdf[r][0], pdf[r][1]} * spl(gsc_p);
                const f2 hi = f2{pdf[r][2], pdf[r][3]} * spl(gsc_p);
                __builtin_nontemporal_store(f4{lo.x, lo.y, hi.x, hi.y}, (f4*)(rowp + 64 * r + voff));
            }
        } else if (full_p) {
            // R = 8: rows through LDS, half a row (blocks 4h .. 4h+3, 256 B) at a
            // time: the D layout gives each lane 16 B of ONE sample per block,
            // i.e. 64-B row segments per store (measured 230 vs 180 us with
            // whole lines); staged, every store writes four contiguous 256-B
            // half rows.  16-B chunk c of row i sits at chunk c ^ i (conflict-
            // free writes and reads).
            // (the empty asm statements: the offset's zero extension stays in
            // this block, where instruction selection can fold it into the
            // store's SGPR-base form -- hoisted out of the loop it costs a
            // 64-bit add per tile -- and rows 8 .. 15 get a scalar base of
            // their own, since the eight constants, rows 4 i and half h, do
            // not all fit the store's 13-bit offset)
            unsigned vo = voff8;
            asm volatile("" : "+v"(vo));
            unsigned up = 8 * (16 * R) * 4;
            asm volatile("" : "+s"(up));
            char* const upper = rowp + up;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int r = (4 * h + rr) % R;
                    const f2 lo = f2{pdf[r][0], pdf[r][1]} * spl(gsc_p);
                    const f2 hi = f2{pdf[r][2], pdf[r][3]} * spl(gsc_p);
                    st[col * 16 + ((4 * rr + g) ^ col)] = f4{lo.x, lo.y, hi.x, hi.y};
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rw = g + 4 * i, ch = col;
                    const f4 v = st[rw * 16 + (ch ^ rw)];
                    __builtin_nontemporal_store(v, (f4*)((i < 2 ? rowp : upper) + vo + (4 * (i & 1) * (16 * R) + 64 * h) * 4));
                }
                __builtin_amdgcn_wave_barrier();
            }
        } else if (col < rows_p) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float o = gsc_p != 0.0f ? pdf[r][j] * gsc_p : 0.0f;
                    if (16 * r + 4 * g + j < K) __builtin_nontemporal_store(o, (float*)(rowp + (16 * r + j) * 4 + voff));
                }
        }
    };

    // prologue: the first kFeatAhead tiles' features in flight
#pragma unroll
    for (int a = 0; a < kFeatAhead; ++a) dma(a, a);
    unsigned hist = 0;   // bit j: the flush j iterations back was full
    unsigned tlow = (unsigned)s0;   // the tile's first sample, low bits
    for (int it = 0; it < nit; ++it, tlow += (unsigned)step) {
        const int slot = it % kFeatSlots;
        dma(it + kFeatAhead, (it + kFeatAhead) % kFeatSlots);   // clamped past the end
        if (rowp != nullptr) hist = (hist << 1) | (full_p ? 1u : 0u);
        flush();                                                       // tile t - step's rows
        const int k = it < kFeatAhead + 1 ? it : kFeatAhead + 1;
        const unsigned need = (1u << k) - 1u;
        f4 fa, fb;   // x0 x1 x2 x3 and x4 x5 hpdf flags of sample col
        read_feat_counted<R>(k, (hist & need) == need, ring_lds + (unsigned)slot * (kFeatSlotU4 * 16u) + 16u * col,
                             fa, fb);
        const float P3[3] = {fa.x, fa.y, fa.z};
        const float D3[3] = {fa.w, fb.x, fb.y};
        // d == 0 fails every log map (mvtn.h:152-154)
        const bool dzero = D3[0] == 0.0f && D3[1] == 0.0f && D3[2] == 0.0f;
        // the tile's rows below s1 (wave-uniform) and the sample this lane's
        // record holds (the DMA's clamp); its flag byte's place in the dword
        // needs the low address bits only
        const int rows = it < jfull ? 16 : rows_last;
        const unsigned cc = (unsigned)(col < rows ? col : rows - 1);
        const unsigned fsh = (((unsigned)(uintptr_t)s.isDiffuse + tlow + cc) & 3u) << 3;
        const bool dif = has_d && ((fbits(fb.w) >> fsh) & 0xffu) != 0u;
        const float hp = has_h ? fb.z : 0.0f;
        const bf8 Bd = a_frag(D3, g, false);
        const bf8 Bs = pfrag(P3);

        // the normaliser's lane partials: two independent packed chains (rows
        // j, j + 1 and j + 2, j + 3), so no product waits on the previous add
        f2 acc = f2{0.0f, 0.0f}, acc2 = f2{0.0f, 0.0f};
        uint32_t cbits = 0;
        auto pair_math = [&](int r, auto rare, const f4 (&D)[8], const f4& dp) __attribute__((always_inline)) {
            constexpr bool RARE = decltype(rare)::value;
            if constexpr (!RARE)
                cbits = __builtin_elementwise_max(
                    cbits, __builtin_elementwise_max(__builtin_elementwise_max(fbits(D[0][0]), fbits(D[0][1])),
                                                     __builtin_elementwise_max(fbits(D[0][2]), fbits(D[0][3]))));
            f2 p[2];
            pdf_quad<RARE>(D[0], D[1], D[2], D[3], D[4], D[5], D[6], D[7], dp, p);
            pdf[r][0] = p[0].x;
            pdf[r][1] = p[0].y;
            pdf[r][2] = p[1].x;
            pdf[r][3] = p[1].y;
            acc = padd(acc, p[0]);
            acc2 = padd(acc2, p[1]);
        };
#if defined(SDMM_SPLIT_DIAG_STOREONLY)
        // diagnostic ceiling (tools/build_variant.sh "-DSDMM_SPLIT_DIAG_STOREONLY"):
        // the same DMA, row staging and stores with no matrix or pair math; the
        // rows are not responsibilities
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pdf[r][j] = P3[j & 1] + D3[j >> 1] + (float)(16 * r + j);
                acc.x += pdf[r][j];
            }
#else
        {
            // pipelined over the blocks: block r + 1's fragments are read from
            // LDS while block r's pair math runs
            bf8 F[2][8];
            f4 dp[2];
            frags(0, F[0], dp[0]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                f4 D[8];
#ifdef SDMM_SPLIT_DIAG_ONEFRAG
                // diagnostic ceiling (tools/build_variant.sh "-DSDMM_SPLIT_DIAG_ONEFRAG"):
                // block 0's fragments and detInv pi quad, read once per tile,
                // serve all R blocks -- 8 fragment reads per tile instead of
                // 8 R, the same matrix and pair math; the rows are not
                // responsibilities.  (The empty asm: the registers are opaque
                // per block, so the R identical blocks are not folded into one.)
#pragma unroll
                for (int f = 0; f < 8; ++f) asm volatile("" : "+v"(F[0][f]));
                asm volatile("" : "+v"(dp[0]));
                forms(F[0], Bs, Bd, D);
                __builtin_amdgcn_sched_barrier(0);
                pair_math(r, Tag<false>{}, D, dp[0]);
#else
                forms(F[r & 1], Bs, Bd, D);
                __builtin_amdgcn_sched_barrier(0);
                pair_math(r, Tag<false>{}, D, dp[r & 1]);
                if (r + 1 < R) frags(r + 1, F[(r + 1) & 1], dp[(r + 1) & 1]);
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#endif
        // rare angle case anywhere in the tile (c < -0.9999995; its bits,
        // unsigned, exceed those of -0.9999995f) or a NaN: redo the tile with
        // the reference's quirks (wave-uniform, a few tiles per launch)
        const bool odd = cbits > __builtin_bit_cast(uint32_t, -0.9999995f) || !((acc.x + acc.y) + (acc2.x + acc2.y) >= 0.0f);
        if (__builtin_amdgcn_ballot_w64(odd) != 0) {
            bf8 bd2 = Bd, bs2 = Bs;
            asm volatile("" : "+v"(bd2), "+v"(bs2));
            acc = f2{0.0f, 0.0f};
            acc2 = f2{0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                bf8 F[8];
                f4 dp, D[8];
                frags(r, F, dp);
                forms(F, bs2, bd2, D);
                pair_math(r, Tag<true>{}, D, dp);
            }
        }
        // posterior normalisation of sample col (mixture_model.h:170-191): the
        // lane's 4 R components, then the four lane groups of the sample
        float S = (acc.x + acc.y) + (acc2.x + acc2.y);
        S = rows_sum4(S);
        const float S2 = dif ? fmaf(1.0f - kHeuristicWeight, S, kHeuristicWeight * hp) : S;
        const float inv = __builtin_amdgcn_rcpf(S2);
        const bool fin = __builtin_isfinite(inv) && !dzero;
        gsc_p = fin ? (dif ? inv * (1.0f - kHeuristicWeight) : inv) : 0.0f;
        // a non-finite sum means a non-finite pdf (NaN/inf input): zero rows by select
        const bool bad = __builtin_amdgcn_ballot_w64(!__builtin_isfinite(S)) != 0;
        full_p = rows == 16 && (16 * R == K) && !bad;
        rowp = rowt;
        rows_p = rows;
        rowt += rowstep;
    }
    flush();
    // the ring's last DMAs (clamped tiles past the end) land before the
    // workgroup's LDS is released
    wait_vm<0>();
}

template <int R, int WPB, int OCC>
__global__ void __launch_bounds__(64 * WPB, OCC)
estep_resp_split_kernel(const float* __restrict__ ep, const u4* __restrict__ img, int Kp, int K, SamplesDev s,
                        int64_t n, int64_t nwaves, float* __restrict__ resp) {
    resp_split_body<R, WPB, false>(ep, img, Kp, K, s, n, nwaves, resp);
}

// SDMM_RESP_IMAGE=inline: the A/B and bitwise-test variant
template <int R, int WPB, int OCC>
__global__ void __launch_bounds__(64 * WPB, OCC)
estep_resp_split_inline_kernel(const float* __restrict__ ep, int Kp, int K, SamplesDev s, int64_t n, int64_t nwaves,
                               float* __restrict__ resp) {
    resp_split_body<R, WPB, true>(ep, nullptr, Kp, K, s, n, nwaves, resp);
}

// ---------------------------------------------------------------------------
// Band form at R = 8 (round 9): the coefficient image lives in registers.
//
// resp_split_body re-reads the mixture's whole 64-KB image from LDS for every
// 16-sample tile (64 ds_read_b128 per tile, 4.7 GB of LDS reads per launch at
// N = 2^20).  Here a wave owns a band of COMPONENTS instead: wave w of a
// 4-wave workgroup keeps blocks 2 w and 2 w + 1 (components 32 w .. 32 w + 31:
// 16 fragments = 64 VGPRs, what the F[2][8] double buffer cost, and two
// detInv pi quads) for the whole launch, and the four waves together cover
// K = 128.  The work unit is a super-tile of 64 samples, four 16-sample tiles;
// wave w is the builder and the storer of tile w:
//
//   1. features of its tile from its DMA ring (the counted vmcnt waits of
//      resp_split_body), the sample fragments Bs / Bd into the workgroup's
//      fragment buffer; the lane keeps its sample's hp, dif, dzero.  Barrier X.
//   2. for each of the four tiles: Bs / Bd from the buffer, 16 MFMAs and two
//      pdf_quad blocks against the resident fragments, the unnormalised pdfs
//      straight into the workgroup's row stage ([64 rows][512 B], the wave's
//      128-B band of each row; the rows 528 B apart, so that the eight rows of
//      a write's lane group fall on different banks: conflict-free writes and
//      reads with constant offsets), the lane's partial normaliser (its 8
//      components of the sample, summed as resp_split_body's acc / acc2) into
//      part[tile][w][lane], and a flag per tile where its band holds a rare
//      angle or a NaN.  Barrier A.  A tile that any wave flagged is redone by
//      all four with the reference's quirks, behind one more barrier (a few
//      super-tiles per launch): the scope of resp_split_body's redo, all 128
//      components of the tile's 16 samples.
//   3. rows 16 w .. 16 w + 15: lane (g, col) reads the four waves' partials
//      P0 .. P3 of its own place in tile w and the sample's normaliser is
//      rows_sum4((P0 + P1) + (P2 + P3)) -- the waves first, in that fixed
//      order, then the four lane groups by the two row swaps; the heuristic
//      mix, v_rcp and the selects as in resp_split_body; the 16 row scales
//      pass through 64 B of LDS into the store layout (lane L: row 2 i +
//      (L >> 5) of store i; wave-local, no barrier), and the rows go from the
//      stage, scaled, as 8 stores of two whole 512-B rows each.
//
// Barrier X of the next super-tile also frees the stage.  The unnormalised
// pdfs are resp_split_body's bits; only the normaliser's summation order
// differs (128 non-negative terms: at most 127 2^-24 relative).
constexpr int kBandWaves = 4;
constexpr int kBandRowU4 = 33;   // a stage row: 32 chunks of 16 B and one of padding
constexpr int kBandOcc = 3;   // workgroups per CU = waves per SIMD

// LDS-only workgroup barrier: the row stores in flight stay in flight (no
// vmcnt wait; every exchange between the waves goes through LDS)
__device__ __forceinline__ void band_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <bool INLINE>
__device__ __forceinline__ void resp_band_body(const float* __restrict__ ep, const u4* __restrict__ img, int Kp, int K,
                                               const SamplesDev& s, int64_t n, float* __restrict__ resp) {
    constexpr int R = 8, NC = R * 8 * 64, NF = kFeatSlots * kFeatSlotU4;
    // the carve: the four feature rings (first: LDS-DMA destinations below
    // 64 KB), the fragment buffer (4 tiles x (Bs, Bd) x 64 lanes), the row
    // stage (64 rows x (32 + 1 pad) chunks), the lanes' partial normalisers
    // (4 tiles x 4 waves x 64 lanes), per wave the 16 row scales of its tile
    constexpr int NB = 4 * 2 * 64, NST = 64 * kBandRowU4, NP = 4 * 4 * 64 / 4, NG = 4;
    constexpr int NTOT = kBandWaves * NF + NB + NST + NP + kBandWaves * NG + 1;   // (+ the four redo flags)
    static_assert(kBandOcc * NTOT * 16 <= 163840, "three workgroups' carved LDS blocks exceed the 160 KB of a CU");
    static_assert(kBandWaves * NF * 16 <= 65536, "LDS-DMA destinations stay below 64 KB");
    __shared__ u4 smem[NTOT];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, col = lane & 15;
    u4* const ring = smem + w * NF;
    u4* const fbuf = smem + kBandWaves * NF;
    f4* const stg = (f4*)(fbuf + NB);
    float* const part = (float*)(stg + NST);
    f4* const gsv = stg + NST + NP + w * NG;
    unsigned* const flags = (unsigned*)(stg + NST + NP + kBandWaves * NG);

    // the wave's band, resident: blocks 2 w and 2 w + 1
    bf8 F[2][8];
    f4 dp[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int idx = ((2 * w + b) * 8 + f) * 64 + lane;
            F[b][f] = __builtin_bit_cast(bf8, INLINE ? image_entry(ep, Kp, idx, NC) : img[idx]);
        }
        const int idx = NC + (2 * w + b) * 4 + g;
        dp[b] = __builtin_bit_cast(f4, INLINE ? image_entry(ep, Kp, idx, NC) : img[idx]);
    }

    // Super-tiles dealt round robin over the launch's workgroups (one round of
    // resident ones): workgroup b serves b, b + G, ..., so the rows written at
    // one time are neighbouring 32-KB blocks (a contiguous range per workgroup
    // would repeat the channel aliasing described in resp_split_body).  Every
    // wave of the workgroup runs all nit super-tiles (the barriers); its own
    // tile of the last one may be partial (rows_last rows) or empty.
    const int64_t nsup = (n + 63) >> 6;
    if ((int64_t)blockIdx.x >= nsup) return;
    const int nit = (int)((nsup - 1 - blockIdx.x) / gridDim.x) + 1;
    const int64_t s0 = 64 * (int64_t)blockIdx.x + 16 * w, step = 64 * (int64_t)gridDim.x, s1 = n;
    const int64_t span = s1 - s0;
    const uint64_t whole = (uint64_t)(span - 16);
    const int jfull = span < 16          ? 0
                      : (whole >> 32) == 0 ? (int)((uint32_t)whole / (uint32_t)step) + 1
                                           : (int)(whole / (uint64_t)step) + 1;
    const int64_t tl = s0 + jfull * step;   // the wave's first tile that is not whole
    const int rows_last = tl < s1 ? (int)(s1 - tl) : 0;

    const bool has_h = s.hpdf != nullptr, has_d = s.isDiffuse != nullptr;
    // DMA sources of this lane, as in resp_split_body: sample sl = lane >> 2
    // of the tile, plane pl = lane & 3 of piece 0 and of piece 1
    const int pl = lane & 3, sl = lane >> 2;
    const uintptr_t src0 = (uintptr_t)(pl == 0 ? s.x[0] : pl == 1 ? s.x[1] : pl == 2 ? s.x[2] : s.x[3]);
    const bool byteplane = pl == 3 && has_d;
    const uintptr_t src1 = (uintptr_t)(pl == 0   ? s.x[4]
                                       : pl == 1 ? s.x[5]
                                       : pl == 2 ? (has_h ? s.hpdf : s.x[0])
                                                 : (has_d ? (const float*)s.isDiffuse : s.x[0]));
    const unsigned sh1 = byteplane ? 0 : 2;
    const unsigned ring_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) u4*)ring;
    // The lane's two source addresses run with the wave's tiles: dma() is
    // called for tiles 0, 1, ... in order.  A whole tile reads its own samples
    // and advances the addresses by the step.  Tile jfull (wave-uniform: the
    // end of the wave's run) moves them back once to its samples clamped to
    // the last one, s1 - 1 (tail = s1 - 1 - tl lies in -64 .. 14: the tile is
    // partial or an empty one of the last super-tile), and they stay there for
    // the ring's look-ahead past the end (records that are never used).  No
    // clamped address is kept in registers through the loop.
    uintptr_t dp0 = src0 + ((uintptr_t)(s0 + sl) << 2);
    uintptr_t dp1 = src1 + ((uintptr_t)(s0 + sl) << sh1);
    const int tail = (int)(s1 - 1 - tl);
    auto dma = [&](int j, int slot) __attribute__((always_inline)) {
        if (j == jfull) {
            int t2 = tail;
            asm volatile("" : "+s"(t2));
            const int back = t2 - (lane >> 2) < 0 ? t2 - (lane >> 2) : 0;
            dp0 += (uintptr_t)((intptr_t)back << 2);
            dp1 += (uintptr_t)((intptr_t)back << sh1);
        }
        dma_pair(dp0, dp1 & ~(uintptr_t)3, ring_lds + (unsigned)slot * (kFeatSlotU4 * 16u));
        const unsigned adv = j < jfull ? (unsigned)step : 0u;
        dp0 += adv << 2;
        dp1 += adv << sh1;
    };
    // the low bits of the sample that the lane's record of the wave's last,
    // not whole tile holds (the DMA's clamp)
    const int64_t ilc = tl + col < s1 ? tl + col : s1 - 1;
    const unsigned last_low = (unsigned)ilc;

    auto forms = [&](const bf8 (&Fb)[8], bf8 bs, bf8 bd, f4 (&D)[8]) __attribute__((always_inline)) {
        const f4 z = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int f = 0; f < 8; ++f) D[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fb[f], f < 3 ? bd : bs, z, 0, 0, 0);
    };

    // store phase constants: store i writes rows 2 i and 2 i + 1 of the wave's
    // tile, lane L the 16-B chunk L & 31 of row 2 i + (L >> 5)
    const int hi = lane >> 5, ch = lane & 31;

#pragma unroll
    for (int a = 0; a < kFeatAhead; ++a) dma(a, a);
    unsigned hist = 0;   // bit j: the store phase j + 1 super-tiles back was full (exactly R stores)
    unsigned tlow = (unsigned)s0;
    char* rowt = (char*)(resp + s0 * (int64_t)K);
    const int64_t rowstep = step * (int64_t)K * 4;
    for (int it = 0; it < nit; ++it, tlow += (unsigned)step) {
        // -- 1: the wave's own tile: features, fragments
        const int slot = it % kFeatSlots;
        dma(it + kFeatAhead, (it + kFeatAhead) % kFeatSlots);
        // younger than this tile's DMA: the pieces of the two tiles after it
        // and the store phases of the last k = min(it, kFeatAhead) super-tiles
        const int k = it < kFeatAhead ? it : kFeatAhead;
        const unsigned need = (1u << k) - 1u;
        f4 fa, fb;
        read_feat_counted<R>(k, (hist & need) == need, ring_lds + (unsigned)slot * (kFeatSlotU4 * 16u) + 16u * col,
                             fa, fb);
        const float P3[3] = {fa.x - kOrigin, fa.y - kOrigin, fa.z - kOrigin};
        const float D3[3] = {fa.w, fb.x, fb.y};
        const bool dzero = D3[0] == 0.0f && D3[1] == 0.0f && D3[2] == 0.0f;
        const int rows = it < jfull ? 16 : rows_last;
        const unsigned slow = it < jfull ? tlow + (unsigned)col : last_low;
        const unsigned fsh = (((unsigned)(uintptr_t)s.isDiffuse + slow) & 3u) << 3;
        const bool dif = has_d && ((fbits(fb.w) >> fsh) & 0xffu) != 0u;
        const float hp = has_h ? fb.z : 0.0f;
        fbuf[(2 * w + 0) * 64 + lane] = __builtin_bit_cast(u4, a_frag(P3, g, true));
        fbuf[(2 * w + 1) * 64 + lane] = __builtin_bit_cast(u4, a_frag(D3, g, false));
        band_barrier();   // X: the four tiles' fragments are up; the stage and the partials are free

        // -- 2: the wave's band of all four tiles
        unsigned oddmask = 0;   // bit t: a rare angle or a NaN in the wave's band of tile t
        auto tile = [&](auto rare, int t, bf8 bs, bf8 bd, u4& bsn, u4& bdn) __attribute__((always_inline)) {
            constexpr bool RARE = decltype(rare)::value;
            uint32_t cbits = 0;
            f2 acc = f2{0.0f, 0.0f}, acc2 = f2{0.0f, 0.0f};
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                f4 D[8];
                forms(F[b], bs, bd, D);
                __builtin_amdgcn_sched_barrier(0);
                if (!RARE && b == 1 && t < 3) {
                    // tile t + 1's fragments are read behind tile t's last
                    // MFMAs, under its second block's pair math
                    bsn = fbuf[(2 * t + 2) * 64 + lane];
                    bdn = fbuf[(2 * t + 3) * 64 + lane];
                }
                if constexpr (!RARE)
                    cbits = __builtin_elementwise_max(
                        cbits, __builtin_elementwise_max(__builtin_elementwise_max(fbits(D[0][0]), fbits(D[0][1])),
                                                         __builtin_elementwise_max(fbits(D[0][2]), fbits(D[0][3]))));
                f2 p[2];
                pdf_quad<RARE>(D[0], D[1], D[2], D[3], D[4], D[5], D[6], D[7], dp[b], p);
                stg[(16 * t + col) * kBandRowU4 + (8 * w + 4 * b + g)] = f4{p[0].x, p[0].y, p[1].x, p[1].y};
                acc = padd(acc, p[0]);
                acc2 = padd(acc2, p[1]);
                __builtin_amdgcn_sched_barrier(0);
            }
            const float ls = (acc.x + acc.y) + (acc2.x + acc2.y);
            part[(4 * t + w) * 64 + lane] = ls;
            if constexpr (!RARE) {
                // a rare angle (c < -0.9999995; its bits, unsigned, exceed
                // those of -0.9999995f) or a NaN in the wave's band of the tile
                const bool odd = cbits > __builtin_bit_cast(uint32_t, -0.9999995f) || !(ls >= 0.0f);
                if (__builtin_amdgcn_ballot_w64(odd) != 0) oddmask |= 1u << t;
            }
        };
        {
            u4 bsn = fbuf[lane], bdn = fbuf[64 + lane];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                tile(Tag<false>{}, t, __builtin_bit_cast(bf8, bsn), __builtin_bit_cast(bf8, bdn), bsn, bdn);
        }
        flags[w] = oddmask;
        band_barrier();   // A: all bands of the stage, all partials and the four waves' flags are up

        // -- 3: the wave's own tile: normalise, store
        // (the tile's staged rows are read first: they return under the
        // flags' round trip and the normaliser's chain)
        const f4* const srow = stg + (16 * w) * kBandRowU4;
        const float* const pw = part + (4 * w) * 64 + lane;
        f4 v[8];
        float W0, W1, W2, W3;
        auto staged = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = srow[(2 * i + hi) * kBandRowU4 + ch];
            W0 = pw[0], W1 = pw[64], W2 = pw[128], W3 = pw[192];
        };
        const u4 fl = *(const u4*)flags;
        staged();
        // A tile that any wave flagged is redone by every wave with the
        // reference's quirks -- all 128 components of its 16 samples, the scope
        // of resp_split_body's redo -- behind a barrier of its own
        // (workgroup-uniform: every wave reads the same four flags; a few
        // super-tiles per launch).
        const unsigned un = (unsigned)__builtin_amdgcn_readfirstlane((int)((fl.x | fl.y) | (fl.z | fl.w)));
        if (un != 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (un & (1u << t)) {
                    u4 d0, d1;
                    tile(Tag<true>{}, t, __builtin_bit_cast(bf8, fbuf[(2 * t) * 64 + lane]),
                         __builtin_bit_cast(bf8, fbuf[(2 * t + 1) * 64 + lane]), d0, d1);
                }
            band_barrier();
            staged();
        }
        __builtin_amdgcn_sched_barrier(0);
        const float S = rows_sum4((W0 + W1) + (W2 + W3));
        const float S2 = dif ? fmaf(1.0f - kHeuristicWeight, S, kHeuristicWeight * hp) : S;
        const float inv = __builtin_amdgcn_rcpf(S2);
        const bool fin = __builtin_isfinite(inv) && !dzero;
        const float gsc = fin ? (dif ? inv * (1.0f - kHeuristicWeight) : inv) : 0.0f;
        // a non-finite sum means a non-finite pdf (NaN/inf input): zero rows by select
        const bool bad = __builtin_amdgcn_ballot_w64(!__builtin_isfinite(S)) != 0;
        const bool full = rows == 16 && (16 * R == K) && !bad;
        // the row scales in store order: row r at (r & 1) * 8 + (r >> 1), so
        // the lane's eight rows 2 i + hi are two 16-B reads (the wave's own
        // LDS accesses run in order: no barrier)
        ((float*)gsv)[(col & 1) * 8 + (col >> 1)] = gsc;
        const f4 sa = gsv[2 * hi], sb = gsv[2 * hi + 1];
        const float scl[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
        __builtin_amdgcn_sched_barrier(0);
        if (full) {
            // (the empty asm statements: the offset is formed here, from the
            // lane index, and not kept in a register through the loop)
            unsigned vo = (unsigned)lane;
            asm volatile("" : "+v"(vo));
            vo *= 16u;
            unsigned up = 4 * 2 * (16 * R) * 4;
            asm volatile("" : "+s"(up));
            char* const upper = rowt + up;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f2 sc = spl(scl[i]);
                const f2 lo = f2{v[i].x, v[i].y} * sc, hh = f2{v[i].z, v[i].w} * sc;
                __builtin_nontemporal_store(f4{lo.x, lo.y, hh.x, hh.y},
                                            (f4*)((i < 4 ? rowt : upper) + vo + (i & 3) * (2 * (16 * R) * 4)));
            }
        } else if (rows > 0) {
            // (the opaque K: the element offsets are worked out here, not
            // hoisted out of the loop into 32 more VGPR pairs)
            int Ko = K;
            asm volatile("" : "+s"(Ko));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int rw = 2 * i + hi;
                const float sc = scl[i];
                if (rw < rows) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float o = sc != 0.0f ? v[i][j] * sc : 0.0f;
                        if (4 * ch + j < Ko)
                            __builtin_nontemporal_store(o, (float*)(rowt + ((unsigned)(rw * Ko + 4 * ch + j) << 2)));
                    }
                }
            }
        }
        hist = (hist << 1) | (full ? 1u : 0u);
        rowt += rowstep;
    }
    // the ring's last DMAs (clamped tiles past the end) land before the
    // workgroup's LDS is released
    wait_vm<0>();
}

// (the template arguments name the configuration like estep_resp_split_kernel's:
// R blocks, waves per workgroup, workgroups' waves per SIMD)
template <int R, int WPB, int OCC>
__global__ void __launch_bounds__(64 * WPB, OCC)
estep_resp_split_band_kernel(const float* __restrict__ ep, const u4* __restrict__ img, int Kp, int K, SamplesDev s,
                             int64_t n, float* __restrict__ resp) {
    static_assert(R == 8 && WPB == kBandWaves, "the band form is four waves over K = 128");
    resp_band_body<false>(ep, img, Kp, K, s, n, resp);
}

// SDMM_RESP_IMAGE=inline: the band's fragments built from ep in the prologue
template <int R, int WPB, int OCC>
__global__ void __launch_bounds__(64 * WPB, OCC)
estep_resp_split_band_inline_kernel(const float* __restrict__ ep, int Kp, int K, SamplesDev s, int64_t n,
                                    float* __restrict__ resp) {
    static_assert(R == 8 && WPB == kBandWaves, "the band form is four waves over K = 128");
    resp_band_body<true>(ep, nullptr, Kp, K, s, n, resp);
}

// ---------------------------------------------------------------------------
// Configurations (R = Kp / 16 blocks, waves per workgroup, waves per SIMD).
// The B image takes R x 8 KB of LDS per workgroup.
#ifndef SDMM_SPLIT_R8_WPB   // (overridable for tools/build_variant.sh A/B builds)
#define SDMM_SPLIT_R8_WPB 12
#define SDMM_SPLIT_R8_OCC 3
#endif
#define SDMM_SPLIT_CONFIGS(X) X(1, 4, 4) X(2, 4, 4) X(4, 4, 4) X(8, SDMM_SPLIT_R8_WPB, SDMM_SPLIT_R8_OCC)

// R = 8 (K = 128): the band form (resp_band_body: 4-wave workgroups, three per
// CU, the coefficient image in registers) unless the caller asks for the LDS
// image (lds_image, SDMM_RESP_KERNEL=splitlds: the A/B and comparison
// configuration), which is one 12-wave workgroup per CU at 3 waves per SIMD
// (the 64-KB coefficient image, the 48 KB of half-row stages and the 18 KB of
// feature rings share the LDS).  Round 4 measured 4-wave / 2-per-SIMD and
// 8-wave / 2-per-SIMD workgroups of that form slower.
static bool split_band(int R, bool lds_image) { return R == 8 && !lds_image; }
static void split_cfg(int R, bool lds_image, int* wpb, int* occ) {
    *wpb = 4;
    *occ = 4;
    if (R == 8) {
        *wpb = SDMM_SPLIT_R8_WPB;
        *occ = SDMM_SPLIT_R8_OCC;
    }
    if (split_band(R, lds_image)) {
        *wpb = kBandWaves;
        *occ = kBandOcc;
    }
}

bool estep_resp_split_supported(int Kp) { return Kp % 16 == 0 && Kp / 16 <= 8 && (Kp / 16 & (Kp / 16 - 1)) == 0; }

// bytes of the coefficient image of a Kp-component record
size_t estep_resp_image_bytes(int Kp) { return (size_t)(Kp / 16) * (8 * 64 + 4) * 16; }

// img = the image of ep, in stream order (one thread per 16-B entry)
hipError_t launch_estep_resp_image(const float* ep, int Kp, void* img, hipStream_t st) {
    if (!estep_resp_split_supported(Kp) || !img) return hipErrorInvalidValue;
    const int entries = (Kp / 16) * (8 * 64 + 4);
    hipLaunchKernelGGL(estep_resp_image_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, ep, Kp,
                       (u4*)img);
    return hipGetLastError();
}

// resident_waves: waves of this kernel the device holds at once (the launch
// is one round of them, fewer when n has fewer tiles).  img: the prebuilt
// coefficient image of ep (launch_estep_resp_image), or NULL for the kernel
// that builds it in every workgroup.
hipError_t launch_estep_resp_split(bool lds_image, const float* ep, const void* img, int Kp, int K, const SamplesDev& s,
                                   int64_t n, int64_t resident_waves, float* resp, hipStream_t st) {
    if (!estep_resp_split_supported(Kp) || K > Kp || resident_waves <= 0) return hipErrorInvalidValue;
    const int R = Kp / 16;
    int wpb, occ;
    split_cfg(R, lds_image, &wpb, &occ);
    const int64_t tiles = (n + 15) / 16;
    const int64_t blocks = ((tiles < resident_waves ? tiles : resident_waves) + wpb - 1) / wpb;
    const int64_t waves = blocks * wpb;
    // the kernel steps its addresses by 16 waves samples held in 32 bits
    if (waves >= (int64_t)1 << 26) return hipErrorInvalidValue;
    if (split_band(R, lds_image)) {
        // one round of resident workgroups, fewer when n has fewer super-tiles
        const int64_t sup = (n + 63) / 64, res = resident_waves / kBandWaves > 0 ? resident_waves / kBandWaves : 1;
        const unsigned grid = (unsigned)(sup < res ? sup : res);
        if (img)
            hipLaunchKernelGGL((estep_resp_split_band_kernel<8, kBandWaves, kBandOcc>), dim3(grid), dim3(64 * kBandWaves), 0, st, ep,
                               (const u4*)img, Kp, K, s, n, resp);
        else
            hipLaunchKernelGGL((estep_resp_split_band_inline_kernel<8, kBandWaves, kBandOcc>), dim3(grid), dim3(64 * kBandWaves), 0, st, ep, Kp, K,
                               s, n, resp);
        return hipGetLastError();
    }
#define X(RR, WW, OO)                                                                                          \
    if (R == RR && wpb == WW && occ == OO) {                                                                   \
        if (img)                                                                                               \
            hipLaunchKernelGGL((estep_resp_split_kernel<RR, WW, OO>), dim3((unsigned)blocks), dim3(64 * WW), 0, st, \
                               ep, (const u4*)img, Kp, K, s, n, waves, resp);                                  \
        else                                                                                                   \
            hipLaunchKernelGGL((estep_resp_split_inline_kernel<RR, WW, OO>), dim3((unsigned)blocks), dim3(64 * WW), \
                               0, st, ep, Kp, K, s, n, waves, resp);                                           \
        return hipGetLastError();                                                                              \
    }
    SDMM_SPLIT_CONFIGS(X)
#undef X
    return hipErrorInvalidValue;
}

// resident waves per CU of the configuration
hipError_t estep_resp_split_occupancy(bool lds_image, int Kp, bool inline_image, int* waves_per_cu) {
    const int R = Kp / 16;
    int wpb, occ;
    split_cfg(R, lds_image, &wpb, &occ);
    int blocks = 0;
    if (split_band(R, lds_image)) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &blocks,
            inline_image ? reinterpret_cast<const void*>(&estep_resp_split_band_inline_kernel<8, kBandWaves, kBandOcc>)
                         : reinterpret_cast<const void*>(&estep_resp_split_band_kernel<8, kBandWaves, kBandOcc>),
            64 * kBandWaves, 0);
        *waves_per_cu = blocks * kBandWaves;
        return e;
    }
#define X(RR, WW, OO)                                                                                          \
    if (R == RR && wpb == WW && occ == OO) {                                                                   \
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(                                           \
            &blocks,                                                                                           \
            inline_image ? reinterpret_cast<const void*>(&estep_resp_split_inline_kernel<RR, WW, OO>)          \
                         : reinterpret_cast<const void*>(&estep_resp_split_kernel<RR, WW, OO>),                \
            64 * WW, 0);                                                                                       \
        *waves_per_cu = blocks * WW;                                                                           \
        return e;                                                                                              \
    }
    SDMM_SPLIT_CONFIGS(X)
#undef X
    return hipErrorInvalidValue;
}

const char* estep_resp_split_name(bool lds_image, int Kp, bool inline_image) {
    static thread_local char buf[64];
    int wpb, occ;
    split_cfg(Kp / 16, lds_image, &wpb, &occ);
    snprintf(buf, sizeof buf, "estep_resp_split%s%s_kernel<%d,%d,%d>", split_band(Kp / 16, lds_image) ? "_band" : "",
             inline_image ? "_inline" : "", Kp / 16, wpb, occ);
    return buf;
}

}  // namespace sdmm
