// dcn3_kernels.hip -- fused modulated-DCN forward, third generation (gfx950).
//
// Same decomposition as dcn_fwd2_kernel (dcn2_kernels.hip): out[Co, px] = W[Co, (tap, c)] * col[(tap, c), px] with the
// column values built by the lane the matrix core expects them from, never stored anywhere.  What changed follows
// the SQ counters of the second generation (profiles/r02_dcn_pmc.md): 188 VALU instructions per wave and k-step
// against 6 MFMAs, 43 % of the wave time parked in s_waitcnt/s_barrier around two serial staging round trips per
// 16-channel chunk.
//   * The LDS x tile is ZERO outside the image, so every validity rule of the reference's bilinear sampler
//     (kernel.cu:467-497: corners outside [0,H-1]x[0,W-1] contribute 0; whole sample 0 unless -1 < y < H, -1 < x < W,
//     :618) is implied by reading the tile: a sample whose 2x2 footprint lies inside the tile needs no per-corner
//     masks, clamps or range tests at all -- one unsigned compare per axis decides "inside the tile".
//   * Sampling runs in tile coordinates; the modulation mask is folded into the row weights (6 multiplies/subtracts
//     for the four corner weights instead of 4 + 8), sigmoid uses v_exp/v_rcp directly.
//   * Weight slice and x tile of a chunk are requested together (one L2/HBM round trip per chunk, not two).
//   * Samples that leave the tile (|offset| > R) still fall back to per-lane global gathers with the full rule set.
// Geometry: stride 1, dilation 1, groups of >= 8 channels (what EDVR / TDAN instantiate); everything else keeps the
// second-generation kernel.
#include "dcn_tile.h"
#include "dcn_plan.h"

#include "timeline.h"

// Timeline slots (timeline.h) of dcn_fwd3_kernel: thread 0 of workgroup (77, 0, 1); read by tools/dcn3_timeline.py
#define F3_TL (blockIdx.x == 77 && blockIdx.y == 0 && blockIdx.z == 1 && threadIdx.x == 0)
enum Fwd3Stamp {
    F3_START = 0,
    F3_CHUNK = 0,        // + 6 * chunk (< 4) + {1: loads issued, 3: x tile in LDS (both R = 3 only), 4: opening barrier passed, 5: 9 taps done, 6: closing barrier passed}
    F3_EPILOGUE = 30,    // output stored
    F3_C1_TAP_END = 40,  // + tap: chunk 1, MFMAs of the tap issued
    F3_C1_TAP = 60,      // + 5 * tap + {0: tap start, 1: corner reads issued, 2: blend (+ far path) done, 3: split done}, chunk 1
};

// The x tile of a 16-channel chunk for an 8 x 32 pixel workgroup: 16 rows x 40 columns x 4 channel quads = 2560 float4
// items = 5 per thread of a 512-thread workgroup.  Item decode is shifts and masks only and four of the five items
// share one address (same position, consecutive quads): the staging of the second generation spent ~9 K cycles per
// chunk just ISSUING its loads (div/mod by 40 and 640, 64-bit address chains) next to co-resident waves in their
// VALU-bound tap loops.
//   items 0..3: position (row tid >> 5, column tid & 31), quad j
//   item  4   : position (row (tid >> 3) & 15, column 32 + (tid & 7)), quad tid >> 7
struct XTile16x40 {
    float v[5][4];
    bool inb0, inb4;
};
__device__ __forceinline__ void xtile16x40_load(XTile16x40& r, const DcnGeom& d, __amdgpu_buffer_rsrc_t x_rs, int c0, int ty0, int tx0, int tid) {
    // x_rs: raw buffer view of this batch element's planes; plane offsets are uniform (SGPR), lane offsets 32-bit bytes
    const unsigned HW4 = 4u * (unsigned)(d.H * d.W);
    {
        const int gy = ty0 + (tid >> 5), gx = tx0 + (tid & 31);
        r.inb0 = gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
        const int gyc = gy < 0 ? 0 : (gy >= d.H ? d.H - 1 : gy), gxc = gx < 0 ? 0 : (gx >= d.W ? d.W - 1 : gx);
        const unsigned off = 4u * (unsigned)(gyc * d.W + gxc);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + 4 * j + e;   // (uniform)
                r.v[j][e] = buf_load(x_rs, off, (unsigned)(c < d.C ? c : d.C - 1) * HW4);
            }
    }
    {
        const int gy = ty0 + ((tid >> 3) & 15), gx = tx0 + 32 + (tid & 7), q = tid >> 7;
        r.inb4 = gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
        const int gyc = gy < 0 ? 0 : (gy >= d.H ? d.H - 1 : gy), gxc = gx < 0 ? 0 : (gx >= d.W ? d.W - 1 : gx);
        const int qe = c0 + 4 * q < d.C ? q : 0;   // (C % 4 == 0: a quad exists entirely or not at all)
        const unsigned off = 4u * (unsigned)(gyc * d.W + gxc) + (unsigned)(4 * qe) * HW4;
#pragma unroll
        for (int e = 0; e < 4; ++e) r.v[4][e] = buf_load(x_rs, off, (unsigned)(c0 + e) * HW4);
    }
}
// zero outside the image and beyond the last channel: the tap loop relies on it
__device__ __forceinline__ void xtile16x40_commit(float4* xt, const XTile16x40& r, const DcnGeom& d, int c0, int tid) {
    constexpr int TC = 40, NPOS = 16 * 40;
    const int p0 = (tid >> 5) * TC + (tid & 31);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int left = r.inb0 ? d.C - (c0 + 4 * j) : 0;
        xt[j * NPOS + p0] = make_float4(left > 0 ? r.v[j][0] : 0.f, left > 1 ? r.v[j][1] : 0.f, left > 2 ? r.v[j][2] : 0.f,
                                        left > 3 ? r.v[j][3] : 0.f);
    }
    const int q = tid >> 7, p4 = ((tid >> 3) & 15) * TC + 32 + (tid & 7);
    const int left = r.inb4 ? d.C - (c0 + 4 * q) : 0;
    xt[q * NPOS + p4] = make_float4(left > 0 ? r.v[4][0] : 0.f, left > 1 ? r.v[4][1] : 0.f, left > 2 ? r.v[4][2] : 0.f,
                                    left > 3 ? r.v[4][3] : 0.f);
}


typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 lo2(const float4& a) { return f32x2{a.x, a.y}; }
__device__ __forceinline__ f32x2 hi2(const float4& a) { return f32x2{a.z, a.w}; }
// s.x * a00 + t.x * a01 + s.y * a10 + t.y * a11 on a pair of channels (VOP3P op_sel / op_sel_hi pick the broadcast half)
__device__ __forceinline__ f32x2 blend4(f32x2 s, f32x2 t, f32x2 a00, f32x2 a01, f32x2 a10, f32x2 a11) {
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(s), "v"(a00));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(r) : "v"(t), "v"(a01));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(r) : "v"(s), "v"(a10));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(r) : "v"(t), "v"(a11));
    return r;
}

// R: halo of the LDS x tile beyond the 3x3 footprint.  R = 3 is the kernel of round 2 (two workgroups per CU).  R = 7 / 11 (one
// workgroup per CU, a 24 x 48 / 32 x 56 tile) are launched next to it when the caller passes probe counters of the offsets
// (rvsr_launch_dcn_fwd3): every candidate returns at once unless the counters select it, so that px-scale offsets sample from LDS
// instead of gathering from global memory lane by lane (3 px mean |offset|: 0.19 -> see profiles/r03_notes.md).  pad + R is a
// multiple of 4 for all three: tile rows start on 16-byte boundaries and the large tiles are staged with 16-byte loads.
// TERMS: terms of the bf16 product (rvsr_common.h: gemm modes): 3 = hi*hi + hi*lo + lo*hi; 2 = without the weights' lo part (that half of
// the weight slice is not fetched); 1 = hi*hi (no lo part of the column values either)
template <int MT, int R, int TERMS = 3>
__global__ __launch_bounds__(512, (MT <= 2 && R == 3) ? 4 : 2) void dcn_fwd3_kernel(const DcnFwdParams p, const bf16x8* __restrict__ wpack) {
    constexpr int TH = 8, NT = TH * 64;
    constexpr int TR = TH + 2 * R + 2, TC = 32 + 2 * R + 2, NPOS = TR * TC;
    constexpr int MP = MT * 32, WVEC = 9 * 2 * MP;  // 16-byte vectors per weight part
    constexpr int WPARTS = TERMS >= 3 ? 2 : 1;      // parts of the weight slice this kernel uses: [hi | lo] or hi only
    constexpr int NWV = (WPARTS * WVEC + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float4* xt = reinterpret_cast<float4*>(smem_raw);           // [2 octets][2 halves][NPOS], zero outside the image
    bf16x8* ws_hi = reinterpret_cast<bf16x8*>(xt + 4 * NPOS);   // [9 taps][2 octets][MP]
    bf16x8* ws_lo = ws_hi + WVEC;
    float* bias_s = reinterpret_cast<float*>(ws_lo + WVEC);     // [MP]
    const DcnGeom& d = p.d;
    if (dcn_halo_not_selected(p.sel)) return;   // (uniform) not the halo the offsets of this call ask for
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
    unsigned sbx, sby, sbz;
    swizzled_block(sbx, sby, sbz, d.swz);
    const int tx = sbx % d.ntx, ty = sbx / d.ntx;
    const int x0 = tx * 32, y0 = ty * TH, mb = sby, b = sbz;
    const int ty0 = y0 - d.pad - R, tx0 = x0 - d.pad - R;  // image coords of tile (0,0); stride 1
    const int nchunks = (d.C + 15) / 16;
    const size_t HW = (size_t)d.H * d.W, hw = (size_t)d.Ho * d.Wo;
    const int oy = y0 + wave, ox = x0 + lo;
    const bool px_ok = oy < d.Ho && ox < d.Wo;
    const size_t pix = (size_t)oy * d.Wo + ox;
    // Sample positions are formed in IMAGE coordinates exactly as the reference does (float(h_in + i) + offset,
    // kernel.cu:594-616) so that floor() and the fractional weights round identically; only the integer corner is
    // moved into tile coordinates.
    const float by = (float)(oy - d.pad), bx = (float)(ox - d.pad);

    // raw buffer views of this batch element's offset / mask planes (rvsr_launch_dcn_fwd3 checks that they span < 4 GB)
    const __amdgpu_buffer_rsrc_t off_rs = buf_view(d.offset + (size_t)b * d.off_bs);
    const __amdgpu_buffer_rsrc_t msk_rs = buf_view(d.mask + (size_t)b * d.mask_bs);
    const __amdgpu_buffer_rsrc_t x_rs = buf_view(d.x + (size_t)b * d.C * HW), out_rs = buf_view(p.out + (size_t)b * d.Co * hw);
    const __amdgpu_buffer_rsrc_t x2g_rs = buf_view_2g(d.x + (size_t)b * d.C * HW);   // (large tiles: bit 31 of a lane offset = "reads zero")

    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = zero16();

    RVSR_STAMP(F3_TL, F3_START);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int c0 = chunk * 16;
        const int cb8 = c0 + 8 * hi;              // first channel of this lane's octet
        const bool oct_ok = px_ok && cb8 < d.C;
        // offsets / mask: buffer loads with a uniform (SGPR) plane offset and a 32-bit per-lane byte offset -- no per-lane
        // 64-bit address arithmetic in the tap loop (three v_lshl_add_u64 per tap otherwise)
        const int g0 = c0 / d.cpg, dg = oct_ok ? cb8 / d.cpg - g0 : 0;
        const unsigned pixc = oct_ok ? (unsigned)pix : 0u;   // lanes without work read pixel 0 (loads stay unconditional)
        const unsigned off_lane = 4u * (pixc + (unsigned)(dg * 18) * (unsigned)hw), msk_lane = 4u * (pixc + (unsigned)(dg * 9) * (unsigned)hw);
        const unsigned off_pl = 4u * (unsigned)(g0 * 18) * (unsigned)hw, msk_pl = 4u * (unsigned)(g0 * 9) * (unsigned)hw, pl = 4u * (unsigned)hw;
        float n_dy = buf_load(off_rs, off_lane, off_pl), n_dx = buf_load(off_rs, off_lane, off_pl + pl), n_m = buf_load(msk_rs, msk_lane, msk_pl);
        {   // weight slice + x tile of the chunk: ALL global loads first, then the LDS writes (one round trip)
            // weight slice: LDS-DMA (global_load_lds_dwordx4: lane l of a wave lands at M0 + 16 l, so a linear copy needs
            // no registers, no ds_write and no wait before the barrier's)
            const bf16x8* src = wpack + ((size_t)mb * nchunks + chunk) * 2 * WVEC;
#pragma unroll
            for (int i = 0; i < NWV; ++i) {
                const int e = tid + i * NT;
                if (e - lane + 63 < WPARTS * WVEC)   // (wave-uniform; WVEC is a multiple of 64)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + e),
                                                     (__attribute__((address_space(3))) void*)(ws_hi + e), 16, 0, 0);
            }
            if constexpr (R == 3) {
                static_assert(R != 3 || (TR == 16 && TC == 40 && NT == 512), "xtile16x40 is written for this tile");
                XTile16x40 xr;
                xtile16x40_load(xr, d, x_rs, c0, ty0, tx0, tid);
                RVSR_STAMP(F3_TL && chunk < 4, F3_CHUNK + 6 * chunk + 1);
                xtile16x40_commit(xt, xr, d, c0, tid);
                RVSR_STAMP(F3_TL && chunk < 4, F3_CHUNK + 6 * chunk + 3);
            } else {
                // item = (quad, row, group of 4 columns): four 16-byte loads (one per channel of the quad) land as the float4s of four
                // positions -- a renaming of registers, no shuffles.  Rows / column groups outside the image and channels beyond C read
                // zeros through the buffer range check (lane offset beyond the 2 GB view); W % 4 == 0 (launcher) keeps a group whole.
                constexpr int TC4 = TC / 4, NITEM = 4 * TR * TC4, NXI = (NITEM + NT - 1) / NT;
                static_assert(TC % 4 == 0, "tile rows are whole 16-byte groups");
                typedef float f32x4v __attribute__((ext_vector_type(4)));
                const unsigned HW4b = 4u * (unsigned)(d.H * d.W);
                f32x4v xv[NXI][4];
#pragma unroll
                for (int k = 0; k < NXI; ++k) {
                    const int it = tid + k * NT;
                    const int q = it / (TR * TC4), rem = it - q * (TR * TC4);
                    const int r = rem / TC4, g4 = rem - r * TC4;
                    const int gy = ty0 + r, gx = tx0 + 4 * g4;
                    const bool ok = it < NITEM && gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
                    const unsigned off = ok ? 4u * (unsigned)(gy * d.W + gx) : 0x80000000u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = c0 + 4 * q + e;
                        xv[k][e] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(x2g_rs, (int)(c < d.C ? off : 0x80000000u),
                                                                                                  (int)((unsigned)(c < d.C ? c : 0) * HW4b), 0));
                    }
                }
#pragma unroll
                for (int k = 0; k < NXI; ++k) {
                    const int it = tid + k * NT;
                    if (it < NITEM) {
                        const int q = it / (TR * TC4), rem = it - q * (TR * TC4);
                        const int r = rem / TC4, g4 = rem - r * TC4;
                        float4* dst = xt + q * NPOS + r * TC + 4 * g4;
                        dst[0] = make_float4(xv[k][0].x, xv[k][1].x, xv[k][2].x, xv[k][3].x);
                        dst[1] = make_float4(xv[k][0].y, xv[k][1].y, xv[k][2].y, xv[k][3].y);
                        dst[2] = make_float4(xv[k][0].z, xv[k][1].z, xv[k][2].z, xv[k][3].z);
                        dst[3] = make_float4(xv[k][0].w, xv[k][1].w, xv[k][2].w, xv[k][3].w);
                    }
                }
            }
            if (chunk == 0 && tid < MP) {
                const int o = mb * MP + tid;
                bias_s[tid] = (p.bias != nullptr && o < d.Co) ? p.bias[o] : 0.f;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the weight DMA of this wave has landed
        __syncthreads();
        RVSR_STAMP(F3_TL && chunk < 4, F3_CHUNK + 6 * chunk + 4);

        const float4* xq0 = xt + (2 * hi) * NPOS;  // channels cb8..cb8+3 (xq0[NPOS + pos]: cb8+4..cb8+7)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            RVSR_STAMP(F3_TL && chunk == 1, F3_C1_TAP + 5 * tap + 0);
            const float dy = n_dy, dx = n_dx;
            float m = n_m;
            if (tap < 8) {  // (compile-time) prefetch the next tap's offsets/mask under this tap's math
                n_dy = buf_load(off_rs, off_lane, off_pl + (unsigned)(2 * tap + 2) * pl);
                n_dx = buf_load(off_rs, off_lane, off_pl + (unsigned)(2 * tap + 3) * pl);
                n_m = buf_load(msk_rs, msk_lane, msk_pl + (unsigned)(tap + 1) * pl);
            }
            if (d.mask_logit) m = __builtin_amdgcn_rcpf(1.f + __expf(-m));  // (uniform)
            m = oct_ok ? m : 0.f;                                            // lanes without work contribute zeros
            const float yr = (by + (float)(tap / 3)) + dy, xr_ = (bx + (float)(tap % 3)) + dx;
            const float fy = floorf(yr), fx = floorf(xr_);
            const int r0 = (int)fy - ty0, s0 = (int)fx - tx0;   // tile coordinates of the top-left corner
            const float ly = yr - fy, lx = xr_ - fx;
            // 2x2 footprint inside the tile <=> 0 <= r0 <= TR-2 and 0 <= s0 <= TC-2 (NaN/huge offsets fail the test)
            const bool in_tile = (unsigned)r0 < (unsigned)(TR - 1) && (unsigned)s0 < (unsigned)(TC - 1);
            // corner weights (x mask) as two register pairs S = (w00, w10), T = (w01, w11); the four-corner blend of a
            // channel pair is then four packed ops with one weight broadcast each.  Spelled in assembly: left to itself the
            // compiler pairs the first channels ACROSS corners and spends 14 v_mov per tap rearranging registers.
            const float wy1 = ly * m;
            const f32x2 wy = {m - wy1, wy1};
            const f32x2 wt = wy * lx, wsd = wy - wt;
            const int pos = in_tile ? r0 * TC + s0 : 0;
            const float4 a00 = xq0[pos], b00 = xq0[NPOS + pos], a01 = xq0[pos + 1], b01 = xq0[NPOS + pos + 1];
            const float4 a10 = xq0[pos + TC], b10 = xq0[NPOS + pos + TC], a11 = xq0[pos + TC + 1], b11 = xq0[NPOS + pos + TC + 1];
            RVSR_STAMP(F3_TL && chunk == 1, F3_C1_TAP + 5 * tap + 1);
            const f32x2 p0 = blend4(wsd, wt, lo2(a00), lo2(a01), lo2(a10), lo2(a11));
            const f32x2 p1 = blend4(wsd, wt, hi2(a00), hi2(a01), hi2(a10), hi2(a11));
            const f32x2 p2 = blend4(wsd, wt, lo2(b00), lo2(b01), lo2(b10), lo2(b11));
            const f32x2 p3 = blend4(wsd, wt, hi2(b00), hi2(b01), hi2(b10), hi2(b11));
            float v[8] = {p0.x, p0.y, p1.x, p1.y, p2.x, p2.y, p3.x, p3.y};
            if (!in_tile && oct_ok) {
                // large offset: this lane gathers its corners from global memory, with the reference's rules spelled out
                // (image coordinates; kernel.cu:467-497,618)
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = 0.f;
                const float y = yr, x = xr_;
                if (y > -1.f && x > -1.f && y < (float)d.H && x < (float)d.W) {
                    const float gy_ = floorf(y), gx_ = floorf(x);
                    const int yi = (int)gy_, xi = (int)gx_;
                    const float qy = y - gy_, qx = x - gx_, py = 1.f - qy, px = 1.f - qx;
                    const bool vy0 = yi >= 0, vy1 = yi + 1 <= d.H - 1, vx0 = xi >= 0, vx1 = xi + 1 <= d.W - 1;
                    const float u00 = (vy0 && vx0) ? py * px * m : 0.f, u01 = (vy0 && vx1) ? py * qx * m : 0.f;
                    const float u10 = (vy1 && vx0) ? qy * px * m : 0.f, u11 = (vy1 && vx1) ? qy * qx * m : 0.f;
                    const int cy0 = vy0 ? yi : 0, cy1 = vy1 ? yi + 1 : d.H - 1;
                    const int cx0 = vx0 ? xi : 0, cx1 = vx1 ? xi + 1 : d.W - 1;
                    const int i00 = cy0 * d.W + cx0, i01 = cy0 * d.W + cx1, i10 = cy1 * d.W + cx0, i11 = cy1 * d.W + cx1;
                    const float* pl = d.x + ((size_t)b * d.C + cb8) * HW;
                    float q00[8], q01[8], q10[8], q11[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {   // all 32 loads in flight together (channel clamped, masked below)
                        const float* q = pl + (size_t)(cb8 + j < d.C ? j : 0) * HW;
                        q00[j] = q[i00]; q01[j] = q[i01]; q10[j] = q[i10]; q11[j] = q[i11];
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        v[j] = cb8 + j < d.C ? u00 * q00[j] + u01 * q01[j] + u10 * q10[j] + u11 * q11[j] : 0.f;
                }
            }
            RVSR_STAMP(F3_TL && chunk == 1, F3_C1_TAP + 5 * tap + 2);
            bf16x8 bh, bl;
            split8(v, bh, bl);
            RVSR_STAMP(F3_TL && chunk == 1, F3_C1_TAP + 5 * tap + 3);
            bf16x8 ah[MT], al[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                ah[mt] = ws_hi[(tap * 2 + hi) * MP + mt * 32 + lo];
                if (TERMS >= 3) al[mt] = ws_lo[(tap * 2 + hi) * MP + mt * 32 + lo];
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma_bf16(ah[mt], bh, acc[mt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) if (TERMS >= 2) acc[mt] = mfma_bf16(ah[mt], bl, acc[mt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) if (TERMS >= 3) acc[mt] = mfma_bf16(al[mt], bh, acc[mt]);
            RVSR_STAMP(F3_TL && chunk == 1, F3_C1_TAP_END + tap);
        }
        RVSR_STAMP(F3_TL && chunk < 4, F3_CHUNK + 6 * chunk + 5);
        __syncthreads();
        RVSR_STAMP(F3_TL && chunk < 4, F3_CHUNK + 6 * chunk + 6);
    }

    if (oy >= d.Ho) return;
    const float neg = p.act == 0 ? 1.f : (p.act == 1 ? 0.f : p.slope);
    if ((d.Wo & 3) == 0 && (((uintptr_t)p.out) & 15) == 0) {   // (uniform)
        // 16-byte stores: a 4x4 transpose inside every quad of lanes turns "lane = pixel, 4 registers = 4 consecutive channels"
        // into "lane = channel, 4 consecutive pixels" (dword stores are store-issue-bound: 32 per lane, ~7.5 K cycles per tile)
        const int j = lo & 3, col4 = x0 + (lo & ~3);
        const bool col_ok = col4 < d.Wo;   // Wo % 4 == 0: the float4 is entirely inside or outside
        const unsigned lane_off = 4u * ((unsigned)(4 * hi + j) * (unsigned)hw + (unsigned)oy * d.Wo + col4);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float r0 = acc[mt][4 * rg + 0], r1 = acc[mt][4 * rg + 1], r2 = acc[mt][4 * rg + 2], r3 = acc[mt][4 * rg + 3];
                quad_transpose4(r0, r1, r2, r3, lo);
                const int ol = mt * 32 + 8 * rg + 4 * hi + j;
                const int o = mb * MP + ol;
                const float bb = bias_s[ol];
                float4 v = make_float4(r0 + bb, r1 + bb, r2 + bb, r3 + bb);
                v.x = v.x > 0.f ? v.x : v.x * neg; v.y = v.y > 0.f ? v.y : v.y * neg;
                v.z = v.z > 0.f ? v.z : v.z * neg; v.w = v.w > 0.f ? v.w : v.w * neg;
                // (channel-group offset added on the vector side, not passed as the store's SGPR soffset: conv2_epilogue_v4 has the reason)
                if (col_ok && o < d.Co) buf_store4(out_rs, lane_off + 4u * (unsigned)(mb * MP + mt * 32 + 8 * rg) * (unsigned)hw, 0u, v);
            }
        }
    } else {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ol = mt * 32 + drow(r, hi);
                const int o = mb * MP + ol;
                const bool ok = ox < d.Wo && o < d.Co;
                const int oc = ok ? o : 0;
                float v = acc[mt][r] + bias_s[ol];
                v = v > 0.f ? v : v * neg;
                if (ok) p.out[((size_t)b * d.Co + oc) * hw + pix] = v;
            }
        }
    }
    RVSR_STAMP(F3_TL, F3_EPILOGUE);
}

template <int MT, int R, int TERMS>
static int launch_dcn_fwd3(const DcnFwdParams& p, const DcnFwdPlan& q, size_t lds, const bf16x8* wpack, hipStream_t st) {
    auto k = dcn_fwd3_kernel<MT, R, TERMS>;
    if (set_lds(k, lds)) FAIL(RVSR_ERR_LAUNCH, "dcn_fwd3: cannot reserve %zu B of LDS", lds);
    hipLaunchKernelGGL(k, dim3(q.gx, q.gy, q.gz), dim3(512), lds, st, p, wpack);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) FAIL(RVSR_ERR_LAUNCH, "dcn_fwd3 launch: %s", hipGetErrorString(e));
    return RVSR_OK;
}

// `wpack`: the image pack_weights_kernel(mode 0, CCG 1) wrote for the plan's MT.  One launch per candidate halo of the plan; with more than
// one, each reads the counters of dcn_offset_probe2_kernel for this call's offsets at `probe` and returns at once unless it is the selected one.
int rvsr_launch_dcn_fwd3(const DcnFwdParams& p_in, const DcnFwdPlan& q, const void* wpack, const unsigned* probe, hipStream_t st) {
    DcnFwdParams p = p_in;
    const bf16x8* wp = (const bf16x8*)wpack;
    for (int k = 0; k < q.ncand; ++k) {
        const DcnHaloCand& c = q.cand[k];
        p.sel = dcn_cand_sel(c, probe);
        int rc = RVSR_ERR_LAUNCH;
#define FWD3(MT, R, NT) case (MT * 100 + R) * 10 + NT: rc = launch_dcn_fwd3<MT, R, NT>(p, q, c.lds, wp, st); break
#define FWD3_TERMS(MT, R) FWD3(MT, R, 3); FWD3(MT, R, 2); FWD3(MT, R, 1)
        switch ((q.mt * 100 + c.halo) * 10 + q.nt) {   // the kernels that are built
            FWD3(1, 3, 3); FWD3(1, 7, 3); FWD3(1, 11, 3);
            FWD3_TERMS(2, 3); FWD3_TERMS(2, 7); FWD3_TERMS(2, 11);
            FWD3_TERMS(4, 3); FWD3_TERMS(4, 7);
            default: FAIL(RVSR_ERR_LAUNCH, "dcn_fwd3: no kernel <%d, %d, %d>", q.mt, c.halo, q.nt);
        }
#undef FWD3_TERMS
#undef FWD3
        if (rc != RVSR_OK) return rc;
    }
    return RVSR_OK;
}
