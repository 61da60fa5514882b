// resize_kernels.hip -- MATLAB's antialiased bicubic imresize at the factors 1/2, 2, 1/4, 4 on uint8 frames, in exact integers (gfx950).
// The reference's Vimeo-90K runs read a second copy of the data set, vimeo_septuplet_BIx2_same, that
// codes/scripts/generate_LR_BI_Vimeo90K.m:28 writes as imresize(imresize(img, 1/2, 'bicubic'), 2, 'bicubic') + imwrite;
// codes/data/util.py:511-710 is the reference's own port of that imresize.  Here the LQ crop is computed from the GT bytes of a window
// around the crop (include/realvsr_hip.h, section 13):
//   src u8 [image][Hw][Ww][C], a window of each frame, ANY byte alignment (plain byte loads)
//   SAME: dst u8 [image][S_h][S_w][C]           = the whole-frame chain (shrink by S, enlarge by S, rounded once) at the crop
//   DOWN: dst u8 [image][S_h / S][S_w / S][C]   = the shrunk frame at the crop
//   crop (optional) u8 [image][S_h][S_w][C]     = the window's own bytes at the crop (the GT), from the tile that is staged anyway
// Every normalised weight of the cubic (a = -0.5; stretched by S when shrinking) is k / 2^n at these factors (the tables below; the
// host asserts their sums), so a value is N / 2^b with N an integer sum over the bytes, and the stored byte is
// clamp(floor((N + 2^(b-1)) / 2^b), 0, 255): b = 16 / 24 for DOWN at S = 2 / 4, 30 / 44 for SAME.  The intermediate image is never
// rounded (MATLAB's is a double).  tests/bicubic_reference.py is the same definition in numpy; the kernel equals it with ==.
//
// A workgroup owns one T x T tile of dst of one image: T = 32 (SAME) or 16 (DOWN).  Four separable integer passes through LDS:
//   stage   the NR x NR source pixels under the tile's NM x NM intermediate pixels, as bytes; row / column r of the stage is the frame's
//           reflect(R0 + r), read at the window's clamp(. - wy, 0, Hw - 1) -- EVERY global read goes through that clamp, so no
//           geometry, however wrong, reads outside src
//   V       shrink vertically:   V[m][x]  = sum_t dn[t] stage[S m + t][x]                 int32 (|V| <= 255 * sum|dn| = 1 224 000)
//   I       shrink horizontally: I[m][n]  = sum_t dn[t] V[m][S n + t]                     int32 at S = 2 (255 * 304^2 = 23 566 080),
//                                                                                         int64 at S = 4 (255 * 4800^2 > 2^31)
//   DOWN stores round(I).  SAME goes on:
//   U       enlarge vertically:  U[y][n]  = sum_t up[y % S][t] I[y / S + first + t][n]    int64 (255 * 304^2 * 152 > 2^31 already)
//   out     enlarge horizontally, round, clamp, store                                     int64 (|N| < 2^53)
// REFLECTION happens in the stage alone.  The frame is continued by symmetric reflection (-1 -> 0, L -> L - 1), periodically; the
// shrinking taps are symmetric, so the intermediate image computed from the continued frame at m = -1, -2 (or Lm, Lm + 1) IS the
// intermediate image reflected at its own border, which is what the enlarging stage of the whole-frame chain reads there.  Frames
// with an edge below 2 S, where the reference's single reflection would no longer do, are refused by the entry point.
// Every store goes to an element of dst / crop that the tile owns.
#include <type_traits>

#include "glue_common.h"

// ---------------------------------------------------------------- the tap tables (host and device)
// shrinking by S: output j reads the 4 S inputs S j - 3 S / 2 + t with weights dn[t] / DN
constexpr int bic_dn(int S, int t) {
    constexpr int d2[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
    constexpr int d4[16] = {-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7};
    return S == 2 ? d2[t] : d4[t];
}
constexpr int bic_dn_first(int S) { return -3 * S / 2; }
constexpr int bic_dn_log2(int S) { return S == 2 ? 8 : 12; }
// enlarging by S: output S m + p reads the 4 inputs m + first(p) + t with weights up[p][t] / UP
constexpr int bic_up(int S, int p, int t) {
    constexpr int u2[2][4] = {{-3, 29, 111, -9}, {-9, 111, 29, -3}};
    constexpr int u4[4][4] = {{-45, 399, 745, -75}, {-7, 93, 987, -49}, {-49, 987, 93, -7}, {-75, 745, 399, -45}};
    return S == 2 ? u2[p][t] : u4[p][t];
}
constexpr int bic_up_first(int S, int p) { return p < S / 2 ? -2 : -1; }
constexpr int bic_up_log2(int S) { return S == 2 ? 7 : 10; }

constexpr bool bic_sums_ok(int S) {
    int d = 0;
    for (int t = 0; t < 4 * S; ++t) d += bic_dn(S, t);
    bool ok = d == (1 << bic_dn_log2(S));
    for (int p = 0; p < S; ++p) {
        int u = 0;
        for (int t = 0; t < 4; ++t) u += bic_up(S, p, t);
        ok = ok && u == (1 << bic_up_log2(S));
    }
    for (int t = 0; t < 2 * S; ++t) ok = ok && bic_dn(S, t) == bic_dn(S, 4 * S - 1 - t);   // symmetric: what the reflection rule rests on
    return ok;
}
static_assert(bic_sums_ok(2) && bic_sums_ok(4), "bicubic tap tables: every row sums to its power-of-two denominator");

// How far an output's taps reach beyond the output pixel (DOWN: beyond the S x S source pixels of the output), from the tables.
constexpr int bic_halo(int S, bool down) {
    if (down) {   // output j owns rows S j .. S j + S - 1 and reads S j + first .. S j + first + 4 S - 1
        const int lo = -bic_dn_first(S), hi = bic_dn_first(S) + 4 * S - 1 - (S - 1);
        return lo > hi ? lo : hi;
    }
    int reach = 0;
    for (int p = 0; p < S; ++p) {   // output S m + p reads intermediate rows m + first(p) .. + 3, each of which reads as above
        const int lo = -(S * bic_up_first(S, p) + bic_dn_first(S) - p);
        const int hi = S * (bic_up_first(S, p) + 3) + bic_dn_first(S) + 4 * S - 1 - p;
        reach = lo > reach ? lo : reach;
        reach = hi > reach ? hi : reach;
    }
    return reach;
}
static_assert(bic_halo(2, false) == 7 && bic_halo(2, true) == 3 && bic_halo(4, false) == 15 && bic_halo(4, true) == 6,
              "bicubic halos (include/realvsr_hip.h, section 13)");

// ---------------------------------------------------------------- the kernel
template <int S, bool DOWN>
struct bic_shape {
    static constexpr int T = DOWN ? 16 : 32;          // tile edge in dst pixels
    static constexpr int NM = DOWN ? 16 : T / S + 5;  // intermediate pixels per tile edge (SAME: floor((y + T - 1) / S) + 2 - (floor(y / S) - 2) + 1)
    static constexpr int NR = S * NM + 3 * S;         // source pixels under them: S (NM - 1) + 4 S
};

// symmetric reflection into [0, n), continued periodically (each turn of the loop lowers |i| by at least n; one turn in a frame >= 2 S)
__device__ __forceinline__ int bic_reflect(int i, int n) {
    while (i < 0 || i >= n) i = i < 0 ? -1 - i : 2 * n - 1 - i;
    return i;
}

template <int S, bool DOWN, int C>
__global__ void __launch_bounds__(256) bicubic_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                      unsigned char* __restrict__ crop, const int* __restrict__ geom, int frames,
                                                      int Hw, int Ww, int Hf, int Wf, int S_h, int S_w, unsigned tiles_x,
                                                      unsigned tiles) {
    typedef bic_shape<S, DOWN> sh;
    constexpr int T = sh::T, NM = sh::NM, NR = sh::NR, NRC = NR * C, NMC = NM * C;
    constexpr int LOG = S == 2 ? 1 : 2;
    typedef typename std::conditional<S == 2, int, long long>::type mid_t;   // (the bound in the header comment)
    __shared__ unsigned char stage[NR * NRC];
    __shared__ int V[NM * NRC];
    __shared__ mid_t I[DOWN ? 1 : NM * NMC];
    __shared__ long long U[DOWN ? 1 : T * NMC];
    __shared__ int rowmap[NR], colmap[NR];

    const int tid = threadIdx.x;
    const size_t image = blockIdx.x / tiles;
    const unsigned tile = blockIdx.x - (unsigned)image * tiles;
    const int ty = (int)(tile / tiles_x), tx = (int)(tile % tiles_x);
    int wy = 0, wx = 0, y0 = 0, x0 = 0;
    if (geom) {   // (uniform)  clamped into what the sizes admit: a wrong geometry gives wrong bytes, never an access outside the buffers
        const int* g = geom + 4 * (image / (size_t)frames);
        wy = min(max(g[0], 0), Hf - Hw), wx = min(max(g[1], 0), Wf - Ww);
        y0 = min(max(g[2], 0), Hf - S_h), x0 = min(max(g[3], 0), Wf - S_w);
        if (DOWN) y0 &= ~(S - 1), x0 &= ~(S - 1);
    }
    // the tile's first dst pixel in frame (SAME) / intermediate (DOWN) coordinates, its first intermediate and source pixel
    const int Yf0 = y0 + ty * T, Xf0 = x0 + tx * T;
    const int m0 = DOWN ? (y0 >> LOG) + ty * T : (Yf0 >> LOG) - 2, n0 = DOWN ? (x0 >> LOG) + tx * T : (Xf0 >> LOG) - 2;
    const int R0 = S * m0 + bic_dn_first(S), C0 = S * n0 + bic_dn_first(S);

    if (tid < NR) rowmap[tid] = min(max(bic_reflect(R0 + tid, Hf) - wy, 0), Hw - 1);
    else if (tid >= 128 && tid < 128 + NR) colmap[tid - 128] = min(max(bic_reflect(C0 + tid - 128, Wf) - wx, 0), Ww - 1) * C;
    static_assert(NR <= 128, "one thread per staged row and per staged column");
    __syncthreads();

    const unsigned char* img = src + image * (size_t)Hw * Ww * C;
    const size_t row_bytes = (size_t)Ww * C;
    for (int i = tid; i < NR * NRC; i += 256) {
        const int r = i / NRC, cb = i - r * NRC, px = cb / C, c = cb - px * C;
        stage[i] = img[(size_t)rowmap[r] * row_bytes + colmap[px] + c];
    }
    __syncthreads();

    if (crop) {   // the window's own bytes at the crop: rows S_h x S_w of the frame, all inside the stage (no reflection: they are in the frame)
        constexpr int TC = DOWN ? T * S : T;
        const int cy0 = ty * TC, cx0 = tx * TC;   // in crop coordinates
        unsigned char* out = crop + image * (size_t)S_h * S_w * C;
        for (int i = tid; i < TC * TC * C; i += 256) {
            const int y = i / (TC * C), xc = i - y * (TC * C), x = xc / C, c = xc - x * C;
            if (cy0 + y < S_h && cx0 + x < S_w)
                out[((size_t)(cy0 + y) * S_w + (cx0 + x)) * C + c] = stage[(y0 + cy0 + y - R0) * NRC + (x0 + cx0 + x - C0) * C + c];
        }
    }

    for (int i = tid; i < NM * NRC; i += 256) {
        const int m = i / NRC, cb = i - m * NRC;
        const unsigned char* s = stage + (S * m) * NRC + cb;
        int acc = 0;
#pragma unroll
        for (int t = 0; t < 4 * S; ++t) acc += bic_dn(S, t) * (int)s[t * NRC];
        V[i] = acc;
    }
    __syncthreads();

    constexpr int BD = 2 * bic_dn_log2(S);   // DOWN's b
    const int OH = DOWN ? S_h >> LOG : S_h, OW = DOWN ? S_w >> LOG : S_w;
    unsigned char* out = dst + image * (size_t)OH * OW * C;
    for (int i = tid; i < NM * NMC; i += 256) {
        const int m = i / NMC, nc = i - m * NMC, n = nc / C, c = nc - n * C;
        const int* v = V + m * NRC + (S * n) * C + c;
        mid_t acc = 0;
#pragma unroll
        for (int t = 0; t < 4 * S; ++t) acc += (mid_t)bic_dn(S, t) * (mid_t)v[t * C];
        if (DOWN) {
            const int oy = ty * T + m, ox = tx * T + n;
            if (oy < OH && ox < OW) {
                const long long q = ((long long)acc + (1ll << (BD - 1))) >> BD;
                out[((size_t)oy * OW + ox) * C + c] = (unsigned char)min(max(q, 0ll), 255ll);
            }
        } else {
            I[i] = acc;
        }
    }
    if (DOWN) return;
    __syncthreads();

    for (int i = tid; i < T * NMC; i += 256) {
        const int y = i / NMC, nc = i - y * NMC;
        const int Yf = Yf0 + y, p = Yf & (S - 1);
        const mid_t* s = I + ((Yf >> LOG) + bic_up_first(S, p) - m0) * NMC + nc;   // rows 0 .. NM - 4 (bic_shape::NM)
        long long acc = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int w = bic_up(S, 0, t);
#pragma unroll
            for (int q = 1; q < S; ++q) w = p == q ? bic_up(S, q, t) : w;
            acc += (long long)w * (long long)s[t * NMC];
        }
        U[i] = acc;
    }
    __syncthreads();

    constexpr int BS = 2 * (bic_dn_log2(S) + bic_up_log2(S));   // SAME's b
    for (int i = tid; i < T * T * C; i += 256) {
        const int y = i / (T * C), xc = i - y * (T * C), x = xc / C, c = xc - x * C;
        const int oy = ty * T + y, ox = tx * T + x;
        if (oy >= OH || ox >= OW) continue;
        const int Xf = Xf0 + x, p = Xf & (S - 1);
        const long long* s = U + y * NMC + ((Xf >> LOG) + bic_up_first(S, p) - n0) * C + c;
        long long acc = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int w = bic_up(S, 0, t);
#pragma unroll
            for (int q = 1; q < S; ++q) w = p == q ? bic_up(S, q, t) : w;
            acc += (long long)w * s[t * C];
        }
        const long long q = (acc + (1ll << (BS - 1))) >> BS;
        out[((size_t)oy * OW + ox) * C + c] = (unsigned char)min(max(q, 0ll), 255ll);
    }
}

// ---------------------------------------------------------------- host side
extern "C" int rvsr_bicubic_halo(int scale, int mode) {
    if ((scale != 2 && scale != 4) || (mode != RVSR_BIC_SAME && mode != RVSR_BIC_DOWN)) return -1;
    return scale == 2 ? (mode == RVSR_BIC_DOWN ? bic_halo(2, true) : bic_halo(2, false))
                      : (mode == RVSR_BIC_DOWN ? bic_halo(4, true) : bic_halo(4, false));
}

static int bicubic_args(const void* src, const void* dst, const int* geom, size_t samples, int frames, int C, int Hw, int Ww, int Hf,
                        int Wf, int S_h, int S_w, int scale, int mode, unsigned* tiles_x, unsigned* tiles_y, size_t* blocks) {
    if (!src || !dst) FAIL(RVSR_ERR_BAD_ARG, "bicubic_u8: null argument");
    if (samples == 0 || frames <= 0 || Hw <= 0 || Ww <= 0 || Hf <= 0 || Wf <= 0 || S_h <= 0 || S_w <= 0)
        FAIL(RVSR_ERR_BAD_ARG, "bicubic_u8: empty shape (%zu samples, %d frames, window %d x %d, frame %d x %d, crop %d x %d)", samples,
             frames, Hw, Ww, Hf, Wf, S_h, S_w);
    if (C != 1 && C != 3) FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: %d channels (1 or 3)", C);
    if (scale != 2 && scale != 4) FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: scale %d (2 or 4)", scale);
    if (mode != RVSR_BIC_SAME && mode != RVSR_BIC_DOWN) FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: mode %d", mode);
    if (Hf > (1 << 24) || Wf > (1 << 24)) FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: frame %d x %d (edges up to 2^24)", Hf, Wf);
    if (Hf % scale || Wf % scale)
        FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: the %d x %d frame is no multiple of the scale %d (modcrop it first)", Hf, Wf, scale);
    if (Hf < 2 * scale || Wf < 2 * scale)
        FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: the %d x %d frame has an edge below 2 * scale: one reflection no longer suffices", Hf, Wf);
    if (Hw > Hf || Ww > Wf) FAIL(RVSR_ERR_BAD_ARG, "bicubic_u8: the %d x %d window exceeds the %d x %d frame", Hw, Ww, Hf, Wf);
    if (S_h > Hf || S_w > Wf) FAIL(RVSR_ERR_BAD_ARG, "bicubic_u8: the %d x %d crop exceeds the %d x %d frame", S_h, S_w, Hf, Wf);
    if (mode == RVSR_BIC_DOWN && (S_h % scale || S_w % scale))
        FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: DOWN needs a crop that is a multiple of the scale %d, got %d x %d", scale, S_h, S_w);
    // the window has to hold the crop and its halo (the whole frame where that is smaller); with geom == NULL the crop sits at the
    // frame's and the window's origin, so the leading halo is all reflection.  Where the window SITS is the caller's contract (geom is
    // device memory): the kernel clamps every read into the window.
    const int h = rvsr_bicubic_halo(scale, mode), lead = geom ? h : 0;
    const int need_h = S_h + lead + h < Hf ? S_h + lead + h : Hf, need_w = S_w + lead + h < Wf ? S_w + lead + h : Wf;
    if (Hw < need_h || Ww < need_w)
        FAIL(RVSR_ERR_BAD_ARG, "bicubic_u8: the %d x %d window does not cover the %d x %d crop and its halo of %d (%d x %d)", Hw, Ww, S_h,
             S_w, h, need_h, need_w);
    const int T = mode == RVSR_BIC_DOWN ? bic_shape<2, true>::T : bic_shape<2, false>::T;
    const int OH = mode == RVSR_BIC_DOWN ? S_h / scale : S_h, OW = mode == RVSR_BIC_DOWN ? S_w / scale : S_w;
    *tiles_y = (unsigned)((OH + T - 1) / T), *tiles_x = (unsigned)((OW + T - 1) / T);
    const size_t tiles = (size_t)*tiles_y * *tiles_x;
    if (tiles > 0x7fffffffu || samples * (size_t)frames > 0x7fffffffu / tiles)
        FAIL(RVSR_ERR_UNSUPPORTED, "bicubic_u8: %zu images of %zu tiles exceed one launch", samples * (size_t)frames, tiles);
    *blocks = samples * (size_t)frames * tiles;
    return RVSR_OK;
}

extern "C" int rvsr_bicubic_u8(const unsigned char* src, unsigned char* dst, unsigned char* crop, const int* geom, size_t samples,
                               int frames, int C, int Hw, int Ww, int Hf, int Wf, int S_h, int S_w, int scale, int mode, void* stream) {
    static_assert(bic_shape<2, true>::T == bic_shape<4, true>::T && bic_shape<2, false>::T == bic_shape<4, false>::T, "one tile per mode");
    unsigned tiles_x = 0, tiles_y = 0;
    size_t nb = 0;
    const int rc = bicubic_args(src, dst, geom, samples, frames, C, Hw, Ww, Hf, Wf, S_h, S_w, scale, mode, &tiles_x, &tiles_y, &nb);
    if (rc != RVSR_OK) return rc;
    const unsigned tiles = tiles_x * tiles_y;
#define BIC_LAUNCH(SS, DD, CC)                                                                                                      \
    hipLaunchKernelGGL((bicubic_kernel<SS, DD, CC>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src, dst, crop, geom, frames, \
                       Hw, Ww, Hf, Wf, S_h, S_w, tiles_x, tiles)
    // the one place that chooses the kernel: one variant per (scale, mode, C)
    const bool down = mode == RVSR_BIC_DOWN;
    if (scale == 2 && !down && C == 3) BIC_LAUNCH(2, false, 3);
    else if (scale == 2 && !down) BIC_LAUNCH(2, false, 1);
    else if (scale == 2 && C == 3) BIC_LAUNCH(2, true, 3);
    else if (scale == 2) BIC_LAUNCH(2, true, 1);
    else if (!down && C == 3) BIC_LAUNCH(4, false, 3);
    else if (!down) BIC_LAUNCH(4, false, 1);
    else if (C == 3) BIC_LAUNCH(4, true, 3);
    else BIC_LAUNCH(4, true, 1);
#undef BIC_LAUNCH
    RETURN_LAUNCH("bicubic_u8");
}
