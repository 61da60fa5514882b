// dcn_plan.h -- which kernels a deformable-convolution call runs, with what candidates, grids and workspace.
//
// The entries of dcn_kernels.hip validate a call (fill_geom), ask one of the two plan functions below, refuse or hand the plan to the
// launchers in order; the launchers (dcn_kernels.hip, dcn2_kernels.hip, dcn3_kernels.hip, dcn6_kernels.hip) map the plan's template
// coordinates to a kernel in one table each and launch it.  Every eligibility rule, span rule, halo rule and workspace layout of the DCN
// kernels is written here and nowhere else.  The plan functions are pure host code: no HIP call, no pointer dereferenced (addresses are
// only tested for alignment), no environment read (the developer switches arrive as an argument), no side effect --
// rvsr_dcn_pack_forward_plan / rvsr_dcn_pack_backward_plan export them, and rvsr_dcn_fused_takes / rvsr_dcn_probe_samples /
// rvsr_dcn_forward_halo export the three rules the Python glue needs, so that it asks instead of restating one.
#pragma once
#include "dcn_common.h"

// The developer A/B switches of the DCN kernels, read from the environment once per process (rvsr_dcn_switches, dcn_kernels.hip).
struct DcnSwitches {
    int bwd_pair;       // RVSR_DCN_BWD: unset or 7 = dcn_bwdin6 + dcn_bwdw6 (1), 64 = dcn_bwdin6 + dcn_bwdw4 (0); anything else is refused (-1)
    char bwd_text[17];  //   its text, for that refusal
    int bwdin6_halo;    // RVSR_DCN5_HALO: dcn_bwdin6's window; negative (unset: -1) = selected on the device
    int fwd3_halo;      // RVSR_DCN3_HALO: dcn_fwd3's tile halo; negative (unset: -1) = from the probe, the caller's hint, or 3 px
    int bwdw6_wpc;      // RVSR_BWDW6_WG=2: two workgroups of four waves per CU (4-row tiles, 2 px window) instead of one of eight (8-row tiles,
                        //   4 px window) -- the configuration whose run-to-run differences were never explained; kept selectable so that the
                        //   determinism test covers it (profiles/r06_notes.md)
};
const DcnSwitches& rvsr_dcn_switches();

// One kernel launch among the candidates of a device-side halo selection: DcnHaloSel without the pointer (-1 / 0: condition absent).
struct DcnHaloCand {
    int halo, ge, lt, ge2;
    unsigned thr_ge, thr_lt, thr_ge2;
    size_t lds;
};
static inline DcnHaloCand dcn_cand_always(int halo) { return {halo, -1, -1, -1, 0, 0, 0, 0}; }
static inline DcnHaloSel dcn_cand_sel(const DcnHaloCand& c, const unsigned* probe) {
    DcnHaloSel s = dcn_halo_always();
    if (c.ge < 0 && c.lt < 0 && c.ge2 < 0) return s;   // (a single launch reads no counters)
    s.probe = probe;
    s.ge = c.ge; s.lt = c.lt; s.ge2 = c.ge2;
    s.thr_ge = c.thr_ge; s.thr_lt = c.thr_lt; s.thr_ge2 = c.thr_ge2;
    return s;
}
// dcn_halo_not_selected on the host, for counters that have been copied there
static inline bool dcn_cand_selected(const DcnHaloCand& c, const unsigned* cnt) {
    return !(c.ge >= 0 && cnt[c.ge] < c.thr_ge) && !(c.ge2 >= 0 && cnt[c.ge2] < c.thr_ge2) && !(c.lt >= 0 && cnt[c.lt] >= c.thr_lt);
}

// ------------------------------------------------------------------------------------------
// geometry

struct DcnRefusal { int rc; const char* msg; };
// What the fused kernels take: 3x3, one group, isotropic stride / pad / dilation, deformable groups that divide the channels into a
// multiple or a divisor of 8, a non-empty output.
static inline DcnRefusal dcn_fused_takes(int B, int C, int H, int W, int Co, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w,
                                         int dil_h, int dil_w, int group, int dg) {
    if (B <= 0 || C <= 0 || Co <= 0 || H <= 0 || W <= 0) return {RVSR_ERR_BAD_ARG, "null/empty argument"};
    if (kh != 3 || kw != 3) return {RVSR_ERR_UNSUPPORTED, "only 3x3 kernels are implemented on the HIP path"};
    if (group != 1) return {RVSR_ERR_UNSUPPORTED, "only group == 1 is implemented on the HIP path"};
    if (stride_h != stride_w || pad_h != pad_w || dil_h != dil_w) return {RVSR_ERR_UNSUPPORTED, "anisotropic stride/pad/dilation"};
    if (dg <= 0 || C % dg) return {RVSR_ERR_BAD_ARG, "channels not divisible by deformable_group"};
    const int cpg = C / dg;
    if (!(cpg % DCN_CC == 0 || DCN_CC % cpg == 0)) return {RVSR_ERR_UNSUPPORTED, "channels per deformable group must divide or be a multiple of 8"};
    if ((H + 2 * pad_h - (dil_h * 2 + 1)) / stride_h + 1 <= 0 || (W + 2 * pad_w - (dil_w * 2 + 1)) / stride_w + 1 <= 0)
        return {RVSR_ERR_BAD_ARG, "empty output"};
    return {RVSR_OK, ""};
}

// Samples of the offset statistic (dcn_offset_probe2_kernel): every 16th row of every offset plane.
static inline size_t dcn_probe_samples(int B, int dg, int Ho, int Wo) { return (size_t)B * (dg * 18) * ((Ho + 15) / 16) * Wo; }

// Geometry of the forward's packed weight image (pack_weights_kernel, mode 0, CCG 1): MT 32-row M tiles per workgroup, chunks of 16 input
// channels, m-blocks of MT * 32 output channels.  The first-generation kernel tiles the output channels the same way.
static inline void dcn_fwd2_geom(int Co, int C, int& mt, int& nchunks, int& nmb) {
    mt = Co <= 32 ? 1 : (Co <= 64 ? 2 : 4);
    nchunks = (C + 15) / 16;
    nmb = (Co + mt * 32 - 1) / (mt * 32);
}
static inline size_t dcn_fwd2_image_bytes(int Co, int C) {
    int mt, nchunks, nmb;
    dcn_fwd2_geom(Co, C, mt, nchunks, nmb);
    return (size_t)nmb * nchunks * 2 * 9 * 2 * (mt * 32) * 16;
}

// ------------------------------------------------------------------------------------------
// forward

// The tile halos dcn_fwd3 is built with: 3 / 7 / 11 px (11 px + the 74 KB weight slice of MT = 4 exceed 160 KB: 7).
static inline int dcn_fwd3_halo(int mt, int halo) { return halo <= 3 ? 3 : (halo <= 7 || mt > 2 ? 7 : 11); }
// The smallest tile that leaves (almost) no sample outside: a k-step in which ANY of a wave's 64 lanes left the tile pays the global
// gather for all of them, and at one workgroup per CU the large tiles hide that latency worse than the small one -- measured
// (profiles/r03_notes.md): a 7 px halo with 10 % of the samples outside is slower than the 3 px halo with 65 % outside.
//   R = 3: at most 8 % of the n offset components beyond 3.5 px (100 c <= 8 n);  R = 7: else, at most 1 % beyond 7.5 px (100 c <= n; or no
//   larger tile);  R = 11: the rest
// (crossovers of the fixed-halo timings at offset std 1.25 / 2.5 / 3.75 / 6.25 px).  `n`: samples behind the counters.  The device selects
// among these candidates (every one is launched, one runs); the host applies dcn_cand_selected to counters of an earlier step.
static inline int dcn_fwd3_cands(size_t n, int mt, DcnHaloCand (&cand)[3]) {
    const unsigned thr3 = (unsigned)(n * 8 / 100) + 1, thr7 = (unsigned)(n / 100) + 1;
    const bool has11 = mt <= 2;
    cand[0] = {3, -1, 1, -1, 0, thr3, 0, 0};
    cand[1] = {7, 1, has11 ? 3 : -1, -1, thr3, thr7, 0, 0};
    cand[2] = {11, 3, -1, 1, thr7, thr7, thr3, 0};   // (a partition: not when R = 3 runs)
    return has11 ? 3 : 2;
}
// The halo a forward of `Co` output channels would select on the device from these counters (DCN_PROBE_COUNTERS of them); 0: no samples.
static inline int dcn_fwd3_halo_of_counters(const unsigned* cnt, size_t n, int Co) {
    if (n == 0) return 0;
    int mt, nchunks, nmb;
    dcn_fwd2_geom(Co, 8, mt, nchunks, nmb);
    DcnHaloCand cand[3];
    const int nc = dcn_fwd3_cands(n, mt, cand);
    for (int k = 0; k < nc; ++k)
        if (dcn_cand_selected(cand[k], cnt)) return cand[k].halo;
    return 0;   // (not reached: the candidates partition the counter space)
}

enum DcnFwdFamily {
    DCN_FWD3 = 0,   // dcn_fwd3_kernel<MT, R, TERMS>: stride 1 / dilation 1 on the bf16 matrix cores, tile halo R
    DCN_FWD2 = 1,   // dcn_fwd2_kernel<8, MT>: the other strides / dilations and frames beyond dcn_fwd3's 32-bit offsets, three terms
    DCN_FWD1 = 2,   // dcn_fwd_kernel<MT, CHS>: exact-f32 MFMA, takes everything
};
struct DcnFwdPlan {
    int rc;             // RVSR_OK, or what the entry returns without launching anything
    char msg[96];
    int family;         // DcnFwdFamily; -1: refused
    int mt;             // 32-row M tiles per workgroup
    int chs;            // dcn_fwd_kernel: 8 = every chunk of 8 channels shares one offset set, 0 = per channel
    int nt;             // terms of a product
    int pack;           // pack_weights_kernel writes the weight image into the workspace first
    int probe_pass;     // dcn_offset_probe2_kernel fills the caller's counters first ...
    size_t nprobe;      //   ... from this many samples
    int ncand;          // dcn_fwd3: launches, each with its selection (one candidate: unconditional)
    DcnHaloCand cand[3];
    unsigned gx, gy, gz;
    size_t lds;         // (dcn_fwd3: of the first candidate)
};

// `x_al16`: the input is 16-byte aligned; `probe`: the caller gave counters to fill; `halo_hint`: act bits 10..13 of rvsr_dcn_pack_forward.
static inline DcnFwdPlan dcn_fwd_plan(const DcnGeom& d, int gemm_mode, bool ws, size_t ws_bytes, bool prepacked, bool x_al16, bool probe,
                                      int halo_hint, const DcnSwitches& sw) {
    DcnFwdPlan q = {};
    q.nt = 3;
    int nchunks, nmb;
    dcn_fwd2_geom(d.Co, d.C, q.mt, nchunks, nmb);
    q.gy = (unsigned)nmb;
    q.gz = (unsigned)d.B;
    const bool c8 = d.cpg % DCN_CC == 0, s1 = d.stride == 1 && d.dil == 1;
    // GEMM mode 1 is exact f32; no workspace, no weight image; a k-octet of the bf16 kernels must lie inside one deformable group
    if (gemm_mode == 1 || !ws || !c8) {
        q.family = DCN_FWD1;
        q.chs = c8 ? 8 : 0;
        q.gx = (unsigned)(d.ntx * ((d.Ho + 3) / 4));
        q.lds = sizeof(float) * (DCN_KC * DCN_NPX + DCN_KC * (q.mt * 32 + 1));
        return q;
    }
    const size_t need = dcn_fwd2_image_bytes(d.Co, d.C);
    if (ws_bytes < need) {
        q.rc = RVSR_ERR_WORKSPACE;
        q.family = -1;
        snprintf(q.msg, sizeof(q.msg), "dcn forward: workspace %zu B < %zu B", ws_bytes, need);
        return q;
    }
    q.pack = !prepacked;
    // the caller's counters: the statistic that selects the tile halo on the device (and that the backward of the same layer reuses)
    q.probe_pass = probe && s1;
    q.nprobe = q.probe_pass ? dcn_probe_samples(d.B, d.C / d.cpg, d.Ho, d.Wo) : 0;
    q.gx = (unsigned)(d.ntx * ((d.Ho + 7) / 8));
    const auto lds_of = [&](int R) { return (size_t)16 * (4 * (8 + 2 * R + 2) * (32 + 2 * R + 2) + 2 * 9 * 2 * q.mt * 32) + sizeof(float) * q.mt * 32; };
    // dcn_fwd3: 32-bit byte offsets into one batch element's x / offset / output planes; larger frames take dcn_fwd2
    const size_t oplanes = (size_t)(d.C / d.cpg) * 18, cmax = (size_t)(d.C > d.Co ? d.C : d.Co), planes = oplanes > cmax ? oplanes : cmax;
    if (!s1 || planes * d.H * d.W * sizeof(float) >= ((size_t)1 << 32)) {
        q.family = DCN_FWD2;
        q.lds = lds_of(D2_R);
        return q;
    }
    q.family = DCN_FWD3;
    if (q.mt >= 2) q.nt = rvsr_gemm_terms_of(gemm_mode);   // reduced-term products (GEMM modes 2 / 3): the kernels of the nf64 / nf128 packs
    // (the 7 / 11 px tiles stage x with 16-byte loads through a 2 GB view)
    const bool big_ok = (d.W % 4 == 0) && x_al16 && (size_t)d.C * d.H * d.W * sizeof(float) < ((size_t)1 << 31);
    if (sw.fwd3_halo >= 0 || !q.probe_pass || !big_ok) {
        // no selection: the switch, else the caller's hint (a halo chosen on the host from an earlier statistic of this layer's offsets), else 3 px
        q.ncand = 1;
        q.cand[0] = dcn_cand_always(dcn_fwd3_halo(q.mt, big_ok ? (sw.fwd3_halo >= 0 ? sw.fwd3_halo : (halo_hint > 0 ? halo_hint : 3)) : 3));
    } else {
        q.ncand = dcn_fwd3_cands(q.nprobe, q.mt, q.cand);
    }
    for (int k = 0; k < q.ncand; ++k) q.cand[k].lds = lds_of(q.cand[k].halo);
    q.lds = q.cand[0].lds;
    return q;
}

// ------------------------------------------------------------------------------------------
// backward

// One batch element's planes are addressed with 32-bit byte offsets (x through a 2 GB view: bit 31 marks the zero padding).
static inline bool dcn_planes_below_2g(const DcnGeom& d) {
    const size_t oplanes = (size_t)(d.C / d.cpg) * 18, planes = oplanes > (size_t)d.C ? oplanes : (size_t)d.C, lim = (size_t)1 << 31;
    return planes * (size_t)d.H * d.W * sizeof(float) < lim && planes * (size_t)d.Ho * d.Wo * sizeof(float) < lim;
}
// The geometries dcn_bwdin6 takes: 8 | channels per deformable group, 8 | C, stride 1, dilation 1, Co <= 128, planes below 2 GB.
static inline bool rvsr_dcn_bwdin6_takes(const DcnGeom& d) {
    return d.cpg % 8 == 0 && d.C % 8 == 0 && d.stride == 1 && d.dil == 1 && d.Co <= 128 && dcn_planes_below_2g(d);
}
static inline int nk6_of(int Co) { return Co <= 16 ? 1 : (Co <= 32 ? 2 : (Co <= 64 ? 4 : 8)); }
// dcn_bwdin6's windows: 2 / 4 / 5 / 8 / 12 px (12 px + the 48 KB weight block of NK = 8 exceed 160 KB: 8)
static inline int dcn_bwdin6_halo(int nk, int halo) { return halo <= 2 ? 2 : (halo <= 4 ? 4 : (halo <= 5 ? 5 : (halo <= 8 || nk > 4 ? 8 : 12))); }
// dcn_bwdin6's share of the backward's workspace, byte offsets: the packed weight image at 0, the per-chunk column norms, the probe's counters
struct Bwdin6Workspace { size_t wnorm, probe, total; };
static inline Bwdin6Workspace bwdin6_workspace(int Co, int C) {
    const size_t nchunks = (size_t)((C + 7) / 8);
    Bwdin6Workspace w;
    w.wnorm = nchunks * 3 * 2 * (2 * nk6_of(Co)) * 32 * 16;
    w.probe = w.wnorm + ((nchunks * 4 + 255) & ~(size_t)255);
    w.total = w.probe + 256;
    return w;
}
// dcn_bwdw6: streams (= partials) of a launch with `wpc` workgroups per CU; 0: more (chunk, 64 output channels) units than the 256 CUs, not covered
static inline int bwdw6_streams(int Co, int C, int wpc, int* nmb_out, int* xcd_out) {
    const int nchunks = C / 8, nmb = (Co + 63) / 64, U = nchunks * nmb;
    if (U <= 0 || U > 256) return 0;
    if (nmb_out) *nmb_out = nmb;
    if (xcd_out) *xcd_out = 32 % U == 0 ? 1 : 0;
    return 256 * wpc / U > 0 ? 256 * wpc / U : 1;
}
// The geometries dcn_bwdw6 takes: dcn_bwdin6's (which writes its gOut operand), at most 256 units, and 32-bit byte offsets into the 64
// gOut planes of a unit.
static inline bool rvsr_dcn_bwdw6_takes(const DcnGeom& d) {
    return rvsr_dcn_bwdin6_takes(d) && bwdw6_streams(d.Co, d.C, 1, nullptr, nullptr) > 0 &&
           (size_t)64 * d.Ho * d.Wo * sizeof(float) < ((size_t)1 << 31);
}
// dcn_bwdw4 addresses 64 gOut planes, 27 offset / mask planes and 8 x planes with 32-bit byte offsets inside 2 GB buffer views
static inline bool dcn_bwdw4_spans_ok(const DcnGeom& d) {
    return (size_t)256 * d.Ho * d.Wo < ((size_t)1 << 31) && (size_t)32 * d.H * d.W < ((size_t)1 << 31);
}
// partial sums of the (P, gy, gz)-grid weight-gradient kernels
static inline int bww_P(int ntiles, int gy, int gz) {
    int P = 256 / (gy * gz);
    if (P < 1) P = 1;
    if (P > ntiles) P = ntiles;
    return P;
}

// The backward's workspace.  [0, base): whichever of these the call needs, each from offset 0 -- the weight-gradient partials of
// dcn_bwdw2 / dcn_bwdw4 ([8P][Co][C * 9 + 1]), dcn_bwdin6's weight image + column norms + probe counters, dcn_bwdw6's partials (sized for
// either schedule).  [handoff_off, total): the gOut^T hand-off of the dcn_bwdin6 / dcn_bwdw6 pair (hi + lo bf16 copy of gOut, one 16-byte
// vector per (row, x tile, 32 output channels, k-step, hi / lo, lane): ~575 MiB at B = 40, Co = 64, 180 x 320); 0 bytes: none.  The query
// has no deformable_groups argument, so it asks rvsr_dcn_bwdw6_takes about the call with the MOST offset planes a batch element can have,
// one deformable group per 8 channels: an upper bound of the planes, hence a buffer only where dcn_bwdw6 takes the call whatever its
// grouping.  The backward writes the hand-off where this is non-zero AND the call itself is taken.
struct DcnBwdWorkspace { size_t base, handoff_off, handoff_bytes, total; };
static inline DcnBwdWorkspace dcn_bwd_workspace(int B, int C, int H, int W, int Co, int stride, int pad, int dil) {
    DcnGeom d = {};
    d.B = B; d.C = C; d.H = H; d.W = W; d.Co = Co; d.stride = stride; d.pad = pad; d.dil = dil;
    d.Ho = (H + 2 * pad - (dil * 2 + 1)) / stride + 1; d.Wo = (W + 2 * pad - (dil * 2 + 1)) / stride + 1;
    d.cpg = 8; d.dg = C / 8;
    const int ntiles = B * ((d.Ho + 3) / 4) * ((d.Wo + 31) / 32);
    const size_t Q = 8 * (size_t)bww_P(ntiles, (Co + 63) / 64, (C + DCN_CC - 1) / DCN_CC);
    const size_t a = sizeof(float) * Q * ((size_t)Co * C * 9 + Co);
    const size_t b6 = bwdin6_workspace(Co, C).total;
    const size_t w6 = (size_t)bwdw6_streams(Co, C, 2, nullptr, nullptr) * ((size_t)Co * C * 9 + Co) * sizeof(float) + 256;
    const size_t m = a > b6 ? (a > w6 ? a : w6) : (b6 > w6 ? b6 : w6);
    DcnBwdWorkspace w;
    w.base = w.handoff_off = (m + 255) & ~(size_t)255;
    w.handoff_bytes = rvsr_dcn_bwdw6_takes(d) ? (size_t)B * (((d.Ho + 7) / 8) * 8) * ((d.Wo + 31) / 32) * (size_t)(2 * ((Co + 63) / 64)) * 4 * 64 * 16 : 0;
    w.total = w.base + w.handoff_bytes;
    return w;
}

enum DcnBwdInFamily {   // input / offset / mask gradient
    DCN_BWDIN_REFUSED = -1,
    DCN_BWDIN_NONE = 0,  // not wanted
    DCN_BWDIN6 = 1,      // dcn_bwdin6_kernel<NK, R, TERMS, ..>: one shared fixed-point LDS window per workgroup, window halo R
    DCN_BWDIN1 = 2,      // dcn_bwd_input_kernel<CHS>: exact-f32 MFMA, takes everything its LDS bound allows
};
enum DcnBwdWFamily {    // weight / bias gradient
    DCN_BWDW_REFUSED = -1,
    DCN_BWDW_NONE = 0,   // not wanted
    DCN_BWDW6 = 1,       // dcn_bwdw6_kernel<R, TERMS, TH>: reads the hand-off dcn_bwdin6 wrote -- the two run as a pair
    DCN_BWDW4 = 2,       // dcn_bwdw4_kernel<NT>: bf16 split products
    DCN_BWDW2 = 3,       // dcn_bwdw2_kernel: exact f32 from an LDS x tile (views / geometries dcn_bwdw4 does not take)
    DCN_BWDW1 = 4,       // dcn_bwd_weight_kernel<0>: exact f32, takes everything
};
struct DcnBwdPlan {
    int rc;             // RVSR_OK, or what the entry returns without launching anything
    char msg[224];
    // input / offset / mask gradient
    DcnBwdInFamily in_family;
    int nk;             // dcn_bwdin6: k-steps of 16 output channels
    int in_nt;          // dcn_bwdin6: terms of a product
    int chs;            // dcn_bwd_input_kernel: 8 / 0 as in the forward
    size_t in_lds;      // dcn_bwd_input_kernel (dcn_bwdin6's follows from <NK, R> at compile time)
    int own_probe;      // dcn_bwdin6 zeroes its counters in the workspace and runs the probe pass itself
    int ncand;          // dcn_bwdin6: launches, each with its selection (one candidate: unconditional)
    DcnHaloCand cand[5];
    int handoff;        // dcn_bwdin6 leaves gOut (x act') behind as the matrix-core operands of dcn_bwdw6 ...
    size_t handoff_off; //   ... at this byte offset of the workspace
    // weight / bias gradient: partials [Q][Co][C * 9] (+ [Q][Co]) at the start of the workspace, reduced in a fixed order afterwards
    DcnBwdWFamily w_family;
    int w_r, w_th;      // dcn_bwdw6: window halo, tile rows (= waves)
    int w_nt;           // dcn_bwdw6 / dcn_bwdw4: terms of a product
    int g_vec;          // dcn_bwdw4 / dcn_bwdw2: the gOut view is 16-byte aligned, its tile may be staged with 16-byte loads
    int ns, nmb, xcd;   // dcn_bwdw6: tile streams, units of 64 output channels, units of a stream on one XCD
    int P, Q, gy, gz;   // grid (P, gy, gz) and partials; dcn_bwdw6: P = Q = ns streams of gy = chunks * nmb units, a grid of P * gy
    size_t w_lds;
};

// want_*: the gradient pointers given; `g_al16` / `g_mode`: the gOut view (and its act' tensor) is 16-byte aligned / its TView mode;
// `probe`: the caller hands the counters of the forward over.
static inline DcnBwdPlan dcn_bwd_plan(const DcnGeom& d, int gemm_mode, bool want_gx, bool want_goff, bool want_gmask, bool want_gw, bool ws,
                                      size_t ws_bytes, bool g_al16, int g_mode, bool probe, const DcnSwitches& sw) {
    DcnBwdPlan q = {};
    const auto refuse = [&](int rc) { q.rc = rc; q.in_family = DCN_BWDIN_REFUSED; q.w_family = DCN_BWDW_REFUSED; return q; };
    const DcnBwdWorkspace lay = dcn_bwd_workspace(d.B, d.C, d.H, d.W, d.Co, d.stride, d.pad, d.dil);
    if (want_gw && (!ws || ws_bytes < lay.total)) {
        snprintf(q.msg, sizeof(q.msg), "dcn backward: workspace %zu B < %zu B", ws_bytes, lay.total);
        return refuse(RVSR_ERR_WORKSPACE);
    }
    if (sw.bwd_pair < 0) {
        snprintf(q.msg, sizeof(q.msg), "dcn backward: RVSR_DCN_BWD=%.16s is not accepted: 7 (or unset) = dcn_bwdin6 + dcn_bwdw6, 64 = dcn_bwdin6 + dcn_bwdw4; "
                 "6 selected dcn_bwdin5, which was removed", sw.bwd_text);
        return refuse(RVSR_ERR_BAD_ARG);
    }
    const bool c8 = d.cpg % DCN_CC == 0;
    const int nty = (d.Ho + 3) / 4;
    // ---- input / offset / mask gradient: dcn_bwdin6 in the split GEMM modes where it takes the geometry and has its workspace
    if (want_gx || want_goff || want_gmask) {
        if (!want_gx || !want_goff || !want_gmask) {
            snprintf(q.msg, sizeof(q.msg), "dcn backward: grad_input/grad_offset/grad_mask must be given together");
            return refuse(RVSR_ERR_BAD_ARG);
        }
        if (gemm_mode != 1 && rvsr_dcn_bwdin6_takes(d) && ws && ws_bytes >= bwdin6_workspace(d.Co, d.C).total) {
            q.in_family = DCN_BWDIN6;
            q.nk = nk6_of(d.Co);
            q.in_nt = q.nk >= 4 ? rvsr_gemm_terms_of(gemm_mode) : 3;   // reduced-term products: the kernels of the nf64 / nf128 packs
            // the pair: where dcn_bwdw6 will take the weight gradient
            q.handoff = want_gw && sw.bwd_pair == 1 && rvsr_dcn_bwdw6_takes(d) && lay.handoff_bytes != 0;
            q.handoff_off = lay.handoff_off;
            if (sw.bwdin6_halo >= 0) {
                q.ncand = 1;
                q.cand[0] = dcn_cand_always(dcn_bwdin6_halo(q.nk, sw.bwdin6_halo));
            } else {
                // A sample beyond the halo costs 32 global gathers + 32 global atomics, a larger halo costs staging and flush work in
                // proportion to its cells (585 / 817 / 945 / 1377 / 2065): switch up as soon as 2 % of the offset components leave the smaller
                // window.  R = 2: few components beyond 2.5 px; R = 4: else, few beyond 3.5 px; R = 5: else, few beyond 5.5; R = 8: else, few
                // beyond 8.5 (or no larger window); R = 12: the rest.  The counters are monotone, so the chain is a partition.
                q.own_probe = !probe;
                const unsigned thr = (unsigned)(dcn_probe_samples(d.B, d.C / d.cpg, d.Ho, d.Wo) * (size_t)2 / 100) + 1;
                const int halos[5] = {2, 4, 5, 8, 12}, counter[5] = {0, 1, 2, 4, -1};   // counter[k]: the one beyond window k
                q.ncand = q.nk <= 4 ? 5 : 4;
                for (int k = 0; k < q.ncand; ++k)
                    q.cand[k] = {halos[k], k ? counter[k - 1] : -1, k + 1 < q.ncand ? counter[k] : -1, -1, thr, thr, 0, 0};
            }
        } else {
            q.in_family = DCN_BWDIN1;
            q.chs = c8 ? 8 : 0;
            const int CoP = (d.Co + 1) & ~1;
            q.in_lds = sizeof(float) * ((size_t)CoP * DCN_NPX + (size_t)CoP * DCN_KC + DCN_KC * DCN_NPX + DCN_CC * 14 * 42);
            if (q.in_lds > 160 * 1024) {
                snprintf(q.msg, sizeof(q.msg), "dcn backward: channels_out %d needs %zu B of LDS", d.Co, q.in_lds);
                return refuse(RVSR_ERR_UNSUPPORTED);
            }
        }
    }
    // ---- weight / bias gradient: dcn_bwdw6 if the hand-off is written, else dcn_bwdw4 / dcn_bwdw2, else the first-generation kernel
    if (!want_gw) return q;
    q.w_nt = 3;
    if (q.handoff) {
        q.w_family = DCN_BWDW6;
        q.w_r = sw.bwdw6_wpc == 2 ? 2 : 4;
        q.w_th = sw.bwdw6_wpc == 2 ? 4 : 8;
        q.w_nt = rvsr_gemm_terms_of(gemm_mode);
        q.ns = bwdw6_streams(d.Co, d.C, sw.bwdw6_wpc, &q.nmb, &q.xcd);
        q.P = q.Q = q.ns;
        q.gy = (d.C / 8) * q.nmb;
        q.gz = 1;
        q.w_lds = (size_t)(q.w_th + 2 * q.w_r + 3) * (32 + 2 * q.w_r + 3) * 32 + (size_t)2 * q.w_th * 8 * 64 * 16;
        return q;
    }
    q.gy = (d.Co + 63) / 64;
    q.gz = (d.C + DCN_CC - 1) / DCN_CC;
    q.P = bww_P(d.B * nty * d.ntx, q.gy, q.gz);
    q.g_vec = g_al16;
    const size_t xtile = (size_t)16 * 2 * (4 + 2 * D2_R + 2) * (32 + 2 * D2_R + 2), f32tiles = sizeof(float) * (DCN_NPX * 65 + DCN_NPX * 97);
    if (!c8) {
        q.w_family = DCN_BWDW1;
        q.Q = 4 * q.P;
        q.w_lds = f32tiles;
    } else if (gemm_mode != 1 && d.stride == 1 && d.dil == 1 && g_mode == 0 && (d.Wo & 3) == 0 && g_al16 && dcn_bwdw4_spans_ok(d)) {
        q.w_family = DCN_BWDW4;
        q.Q = 8 * q.P;
        q.w_nt = rvsr_gemm_terms_of(gemm_mode);
        q.w_lds = xtile + (size_t)2 * (64 + 96) * 272;
    } else {
        q.w_family = DCN_BWDW2;
        q.Q = 8 * q.P;
        q.w_lds = xtile + f32tiles;
    }
    return q;
}
