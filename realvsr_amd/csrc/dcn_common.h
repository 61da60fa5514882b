// dcn_common.h -- what every DCN translation unit shares (dcn_kernels.hip, dcn2_kernels.hip, dcn3_kernels.hip, dcn6_kernels.hip): the
// geometry and parameter blocks of the kernels, the sampling rule, the device-side halo selection, and the launchers' declarations.
// Which kernels a call runs is decided in dcn_plan.h.
#pragma once
#include "rvsr_common.h"

#define DCN_CC 8      // input channels per K chunk
#define DCN_KC 72     // = DCN_CC * 9 column rows per chunk
#define DCN_NPX 128   // pixels per tile (4 rows x 32)
#define D2_R 3        // halo radius (pixels) of the LDS x tile of dcn_fwd2 / dcn_bwdw2 / dcn_bwdw4 beyond the 3x3 footprint (dcn_tile.h)

struct DcnGeom {
    const float* x;       // (B, C, H, W)
    const float* offset;  // (b * off_bs)[(g*18 + 2k + {0:dy,1:dx})][Ho][Wo]
    const float* mask;    // (b * mask_bs)[(g*9 + k)][Ho][Wo]
    size_t off_bs, mask_bs;
    int mask_logit;       // 1: mask holds logits, sigmoid applied here
    int B, C, H, W, Co, Ho, Wo;
    int stride, pad, dil, dg, cpg;
    int ntx;
    int swz;  // XCD-aware workgroup remap on/off
};

struct Samp {
    float w00, w01, w10, w11;  // bilinear corner weights (0 for corners outside the image)
    float ly, lx;
    int i00, i01, i10, i11;    // clamped plane indices (always safe to load)
    float m;                   // modulation mask
    bool inside;
    bool v00, v01, v10, v11;   // corner inside the image
};

// sampling geometry of tap k at output pixel (oy, ox) for deformable group g  (kernel.cu:594-618)
__device__ __forceinline__ Samp dcn_sample(const DcnGeom& d, int b, int g, int k, int oy, int ox) {
    const size_t hw = (size_t)d.Ho * d.Wo;
    const size_t p = (size_t)oy * d.Wo + ox;
    const float* ob = d.offset + (size_t)b * d.off_bs + (size_t)(g * 18 + 2 * k) * hw + p;
    const float dy = ob[0], dx = ob[hw];
    float m = d.mask[(size_t)b * d.mask_bs + (size_t)(g * 9 + k) * hw + p];
    if (d.mask_logit) m = 1.f / (1.f + __expf(-m));
    const float y = (float)(oy * d.stride - d.pad + (k / 3) * d.dil) + dy;
    const float x = (float)(ox * d.stride - d.pad + (k % 3) * d.dil) + dx;
    Samp s;
    s.m = m;
    s.inside = (y > -1.f) && (x > -1.f) && (y < (float)d.H) && (x < (float)d.W);
    s.w00 = s.w01 = s.w10 = s.w11 = 0.f;
    s.ly = s.lx = 0.f;
    s.i00 = s.i01 = s.i10 = s.i11 = 0;
    s.v00 = s.v01 = s.v10 = s.v11 = false;
    if (s.inside) {
        const float fy = floorf(y), fx = floorf(x);
        const int y0 = (int)fy, x0 = (int)fx, y1 = y0 + 1, x1 = x0 + 1;
        const float ly = y - fy, lx = x - fx, hy = 1.f - ly, hx = 1.f - lx;
        s.ly = ly;
        s.lx = lx;
        const bool vy0 = y0 >= 0, vy1 = y1 <= d.H - 1, vx0 = x0 >= 0, vx1 = x1 <= d.W - 1;
        const int cy0 = vy0 ? y0 : 0, cy1 = vy1 ? y1 : d.H - 1, cx0 = vx0 ? x0 : 0, cx1 = vx1 ? x1 : d.W - 1;
        s.i00 = cy0 * d.W + cx0;
        s.i01 = cy0 * d.W + cx1;
        s.i10 = cy1 * d.W + cx0;
        s.i11 = cy1 * d.W + cx1;
        s.v00 = vy0 && vx0;
        s.v01 = vy0 && vx1;
        s.v10 = vy1 && vx0;
        s.v11 = vy1 && vx1;
        s.w00 = s.v00 ? hy * hx : 0.f;
        s.w01 = s.v01 ? hy * lx : 0.f;
        s.w10 = s.v10 ? ly * hx : 0.f;
        s.w11 = s.v11 ? ly * lx : 0.f;
    }
    return s;
}


// Device-side choice among tile halos: every candidate kernel is launched and returns at once unless
//   (ge < 0 || probe[ge] >= thr_ge) && (lt < 0 || probe[lt] < thr_lt)
// probe[0..5] = sampled counts of offset components with |v| > 2.5 / 3.5 / 5.5 / 7.5 / 8.5 / 11.5 px (dcn_offset_probe2_kernel): the
// backward's windows (2 / 5 / 8 / 12 px) use counters 0, 2, 4, the forward's tiles (3 / 7 / 11 px) counters 1, 3, 5.  probe == nullptr: run.
#define DCN_PROBE_COUNTERS 6
//   (ge < 0 || probe[ge] >= thr_ge) && (ge2 < 0 || probe[ge2] >= thr_ge2) && (lt < 0 || probe[lt] < thr_lt)
// (two lower conditions: the candidates of a cascade "A while x < a, else B while y < b, else C" form a partition only if C also
// carries "x >= a" -- a heavy-tailed offset field can have y >= b with x < a, and A and C would both run)
struct DcnHaloSel {
    const unsigned* probe;
    int ge, lt, ge2;
    unsigned thr_ge, thr_lt, thr_ge2;
};
__device__ __forceinline__ bool dcn_halo_not_selected(const DcnHaloSel& s) {
    if (s.probe == nullptr) return false;
    if (s.ge >= 0 && s.probe[s.ge] < s.thr_ge) return true;
    if (s.ge2 >= 0 && s.probe[s.ge2] < s.thr_ge2) return true;
    if (s.lt >= 0 && s.probe[s.lt] >= s.thr_lt) return true;
    return false;
}
static inline DcnHaloSel dcn_halo_always() { DcnHaloSel s; s.probe = nullptr; s.ge = s.lt = s.ge2 = -1; s.thr_ge = s.thr_lt = s.thr_ge2 = 0; return s; }

struct DcnFwdParams {
    DcnGeom d;
    const float* w;     // (Co, C, 3, 3)
    const float* bias;  // nullable
    float* out;         // (B, Co, Ho, Wo)
    int act;
    float slope;
    int prepacked;      // the workspace already holds the packed weight image (rvsr_dcn_pack_weights / rvsr_pack_weights_batched)
    DcnHaloSel sel;     // halo selection on the device (dcn_fwd3_kernel<MT, R>)
};


// The launchers: each takes the plan of the call (dcn_plan.h), maps its coordinates to a kernel and launches; none decides anything.
struct DcnFwdPlan;
struct DcnBwdPlan;
// the sampled offset statistic both DCN directions select their tile halo from (dcn6_kernels.hip); `cnt`: zeroed by the caller
void rvsr_launch_dcn_offset_probe(const DcnGeom& d, unsigned* cnt, hipStream_t st);
// forward (dcn2_kernels.hip, dcn3_kernels.hip): the weight image of dcn_fwd2 / dcn_fwd3 into `wpack`, then one of the two families
void rvsr_launch_dcn_fwd_pack(const DcnFwdParams& p, void* wpack, hipStream_t st);
int rvsr_launch_dcn_fwd2(const DcnFwdParams& p, const DcnFwdPlan& q, const void* wpack, hipStream_t st);
int rvsr_launch_dcn_fwd3(const DcnFwdParams& p, const DcnFwdPlan& q, const void* wpack, const unsigned* probe, hipStream_t st);
// input / offset / mask gradient (dcn6_kernels.hip): one shared fixed-point LDS window per workgroup, lane = (pixel, tap), packed math; its
// weight image, column norms and counters live at the start of `workspace` (bwdin6_workspace); `probe`: the caller's counters or nullptr
int rvsr_launch_dcn_bwdin6(const DcnGeom& d, const DcnBwdPlan& q, const float* weight, const TView& g, float* gx, float* goff, size_t goff_bs,
                           float* gmask, size_t gmask_bs, void* workspace, const unsigned* probe, hipStream_t st);
// weight / bias gradient partials into `part` / `bpart` (nullable): dcn_bwdw6 (dcn6_kernels.hip; column values transposed by the matrix core,
// chunk-major persistent, its gOut operand pre-transposed by dcn_bwdin6 at `agt`), dcn_bwdw4 / dcn_bwdw2 (dcn2_kernels.hip)
int rvsr_launch_dcn_bwdw6(const DcnGeom& d, const DcnBwdPlan& q, const void* agt, float* part, float* bpart, hipStream_t st);
int rvsr_launch_dcn_bwdw2(const DcnGeom& d, const DcnBwdPlan& q, const TView& g, float* part, float* bpart, hipStream_t st);
