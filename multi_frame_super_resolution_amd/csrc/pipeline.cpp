// pipeline.cpp -- burst driver: N raw frames in -> one x-s frame out.
//
// This is the L3 layer the reference lacks for its ImageStackAlignator kernels
// (the order below is reconstructed from the kernels'
// data dependencies; the reference's only working burst driver,
// finalProject/Project/multi_frame_sr.cpp:146-209, drives third-party OpenCV
// code).  Stage letters follow SURVEY.md section 3.3:
//
//   set_reference : A1 half-res RGB, tracking pyramid (gray -> gaussin_filter_1D
//                   prefilter -> 2x box levels), E structure tensor -> smooth ->
//                   ComputeKernelParam, A2+A3 debayered fallback image
//   add_frame     : A1, tracking pyramid, B tile tracking coarse -> fine,
//                   D CreateFlowFieldFromTiles + K Lucas-Kanade iterations,
//                   F ComputeRobustnessMask, G accumulate onto the HR grid
//   finish        : H ApplyWeighting (+fallback) + GammasRGB (+quantise)
//
// The joint shift minimiser (C) is the identity when only (reference, k) pairs
// are measured, which is the per-frame streaming / frame-sharded mode this
// driver implements; it is exposed separately (mfsr_minimizeShifts).
//
// Everything runs on the caller's stream out of the caller's workspace: no
// allocation, no synchronisation, so a whole add_frame chain can be captured in
// a hipGraph.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "common.hpp"
#include "raw_stage.hpp"
#include "stencil_host.hpp"

namespace {

constexpr int kMaxLevels = 4;
constexpr int kMaxTimedLaunches = 4096;
// Per-frame products (flow, certainty mask) live in a ring of kRing slots: a frame's slot stays
// untouched until the warp+fuse that consumes it has run, which with cfg.asyncFuse happens on the
// burst's own stream while the caller's stream already aligns the next frames.
constexpr int kRing = 2 * MFSR_MAX_FUSE_GROUP;  // a group waiting to be fused + the group the fuse stream is reading
// With the burst hold (mfsr_burst_hold_fuse) the complete groups of a burst wait for ONE warp+fuse launch, so their slots must
// outlive the alignment of the groups after them: the ring is max(kRing, min(cfg.frames, kRingMax)) slots, a run-time size.
constexpr int kRingMax = MFSR_MAX_BURST_FUSE;
inline int ring_size(const mfsr_config* c) { return c->frames <= kRing ? kRing : (c->frames < kRingMax ? c->frames : kRingMax); }
constexpr int kMaxUploadRing = 32;

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Img {
    void* ptr = nullptr;
    int pitch = 0;
    int w = 0, h = 0;
};

// what prepare_frame (+ mfsr_preAlignPyramid) makes from one raw frame; nothing of it depends on the reference
struct FrameProducts {
    uint16_t* raw;  // the frame itself where the owner keeps it (frame streams, joint mode); null in Layout
    Img half;       // float3, half res
    Img pyr[8];     // float, factor 1,2,4,.. (index = log2 factor)
    void* prePyr;   // cfg.preAlign: search pyramid
};

// what aligning one moved frame against the reference writes besides its ring slot
struct AlignScratch {
    Img shifts[kMaxLevels];    // float2, tile grids
    Img lkSum[2], lkDiff[2];   // fused LK: (warped + ref) / (warped - ref) handed from iteration to iteration
    mfsr_prealign* preResult;  // cfg.preAlign: the frame's estimate (device memory)
};

// The workspace map.  make_layout writes it, nobody else: which frame a stage works on is an argument of the stage.
struct Layout {
    // geometry
    int W, H, hw, hh, tw, th, hrW, hrH;
    int flowScale;
    int lw[kMaxLevels], lh[kMaxLevels];      // level image dims
    int tcx[kMaxLevels], tcy[kMaxLevels];    // tile counts per level
    int maxFactor;
    // buffers
    // the reference's products; the moved frame's products and scratch of batch position q of a group (frame-batched
    // alignment; frame-by-frame alignment works in [0]); nAlign of each are allocated
    FrameProducts ref, mov[MFSR_MAX_FUSE_GROUP];
    AlignScratch work[MFSR_MAX_FUSE_GROUP];
    int nAlign;
    Img kparam4;                             // float4, tracking res
    Img tensor, tensorTmp, tensorSm;         // float3, tracking res
    Img fallback;                            // float3, W x H
    Img tmpA, tmpB;                          // float, tracking res
    Img flowBuf[2 * kRingMax];               // float2, tracking res: per ring slot the two buffers of the LK ping-pong
    Img maskBuf[kRingMax];                   // float4, half res, one per ring slot (ring_size(cfg) slots are allocated)
    Img maskRaw[MFSR_MAX_FUSE_GROUP];        // cfg.maskErode > 0 only: stage F writes here, the erosion writes the slot's mask
    Img pre[kMaxLevels];                     // float2, tile grids: the unfused tracker's upsampled pre-shifts
    // unfused path scratch
    Img warped, Ix, Iy, It, rawf;
    float *refTiles, *movTiles, *cc, *boxX, *boxY, *sqsum, *dist;
    float* refSq[kMaxLevels];  // fused tracker: sum(ref^2) per tile and level, taken once per reference
    void* preWork;             // global pre-alignment (cfg.preAlign): the search's workspace
    // host-frame bursts (cfg.uploadRing): device slots the library uploads into
    uint16_t* rawRing[kMaxUploadRing];
    uint16_t* refRaw[2];
    // cfg.rawPacking: the packed bytes of upload slot i as they came over the link ([ring], [ring + 1] = the reference slots)
    uint8_t* stage[kMaxUploadRing + 2];
    size_t total;
};

struct Bump {
    char* base;
    size_t off;
    void* take(size_t bytes)
    {
        off = align_up(off, 256);
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
    Img image(int w, int h, int elemBytes)
    {
        Img im;
        im.w = w;
        im.h = h;
        im.pitch = (int)align_up((size_t)w * elemBytes, 64);
        im.ptr = take((size_t)im.pitch * h);
        return im;
    }
};

int validate(const mfsr_config* c)
{
    MFSR_REQUIRE(c != nullptr);
    MFSR_REQUIRE(c->width >= 64 && c->height >= 64 && (c->width % 4) == 0 && (c->height % 4) == 0);
    MFSR_REQUIRE(c->frames >= 1 && c->reference >= 0 && c->reference < c->frames);
    MFSR_REQUIRE(c->scale >= 1 && c->scale <= 8);
    MFSR_REQUIRE(c->levels >= 1 && c->levels <= kMaxLevels);
    MFSR_REQUIRE(c->levelFactor[c->levels - 1] == 1);
    for (int l = 0; l < c->levels; l++) {
        const int f = c->levelFactor[l];
        MFSR_REQUIRE(f >= 1 && f <= 128 && (f & (f - 1)) == 0);
        if (l > 0) MFSR_REQUIRE(c->levelFactor[l] < c->levelFactor[l - 1]);
        MFSR_REQUIRE(c->tileSize[l] >= 4 && c->tileSize[l] <= 128 && c->maxShift[l] >= 1 && c->maxShift[l] <= 15);
        MFSR_REQUIRE(c->tileSize[l] > 2 * c->maxShift[l]);
        if (c->fused) {
            // LDS need of one tile in mfsr_trackTilesFused (template + patch + row sums + distance image) against the CU's
            // 160 KB: fail at create, not at the first add_frame (tileSize >~ 110); cfg.fused = 0 serves larger tiles
            const long long T = c->tileSize[l], S = c->maxShift[l], Lt = T + 2 * S, R = 2 * S + 1;
            if (4 * (T * T + Lt * (Lt + 1) + 1 + Lt * R + R * R + 4) > 160 * 1024) {
                fprintf(stderr, "mfsr: tileSize %d / maxShift %d exceeds the fused tile tracker's LDS budget (use cfg.fused = 0)\n",
                        (int)T, (int)S);
                return MFSR_E_UNSUPPORTED;
            }
        }
    }
    MFSR_REQUIRE(c->lkIterations >= 0 && c->lkHalfWindow >= 0 && c->lkHalfWindow <= 15);
    MFSR_REQUIRE(c->maxVal > 0);
    if (c->preAlign) MFSR_REQUIRE(c->preAlignMaxAngle >= 0.0f && c->preAlignMaxAngle <= 45.0f);
    MFSR_REQUIRE(c->uploadRing == 0 || (c->uploadRing >= 3 && c->uploadRing <= kMaxUploadRing));
    MFSR_REQUIRE(c->pairFrames >= 0 && c->pairFrames <= MFSR_MAX_FUSE_GROUP);
    MFSR_REQUIRE(c->maskErode >= 0 && c->maskErode <= 2);
    // packed host frames: the library's own uploads only, and rows of whole groups
    if (c->rawPacking != MFSR_PACK_NONE) MFSR_REQUIRE(c->uploadRing > 0 && mfsr_packed_row_bytes(c->rawPacking, c->width) > 0);
    return MFSR_OK;
}

Layout make_layout(const mfsr_config* c, char* base)
{
    Layout layout;
    memset((void*)&layout, 0, sizeof(layout));
    Layout* L = &layout;
    Bump b{base, 0};
    L->W = c->width;
    L->H = c->height;
    L->hw = c->width / 2;
    L->hh = c->height / 2;
    L->tw = c->mono ? L->W : L->hw;
    L->th = c->mono ? L->H : L->hh;
    L->flowScale = c->mono ? 1 : 2;
    L->hrW = c->width * c->scale;
    L->hrH = c->height * c->scale;
    L->maxFactor = c->levelFactor[0];
    const int nl = ilog2(L->maxFactor) + 1;

    L->ref.half = b.image(L->hw, L->hh, 12);
    L->mov[0].half = b.image(L->hw, L->hh, 12);
    for (int i = 0; i < nl; i++) {
        L->ref.pyr[i] = b.image(L->tw >> i, L->th >> i, 4);
        L->mov[0].pyr[i] = b.image(L->tw >> i, L->th >> i, 4);
    }
    L->kparam4 = b.image(L->tw, L->th, 16);
    L->tensor = b.image(L->tw, L->th, 12);
    L->tensorTmp = b.image(L->tw, L->th, 12);
    L->tensorSm = b.image(L->tw, L->th, 12);
    L->fallback = b.image(L->W, L->H, 12);
    L->tmpA = b.image(L->tw, L->th, 4);
    L->tmpB = b.image(L->tw, L->th, 4);
    for (int i = 0; i < 2 * kRing; i++) L->flowBuf[i] = b.image(L->tw, L->th, 8);
    for (int i = 0; i < kRing; i++) L->maskBuf[i] = b.image(L->hw, L->hh, 16);
    size_t maxTileFloats = 0, maxTiles = 0, maxDist = 0;
    for (int l = 0; l < c->levels; l++) {
        const int f = c->levelFactor[l];
        L->lw[l] = L->tw / f;
        L->lh[l] = L->th / f;
        L->tcx[l] = L->lw[l] / c->tileSize[l] > 0 ? L->lw[l] / c->tileSize[l] : 1;
        L->tcy[l] = L->lh[l] / c->tileSize[l] > 0 ? L->lh[l] / c->tileSize[l] : 1;
        L->work[0].shifts[l] = b.image(L->tcx[l], L->tcy[l], 8);
        L->pre[l] = b.image(L->tcx[l], L->tcy[l], 8);
        const size_t tiles = (size_t)L->tcx[l] * L->tcy[l];
        const size_t Lt = (size_t)c->tileSize[l] + 2 * c->maxShift[l];
        const size_t R = 2 * (size_t)c->maxShift[l] + 1;
        if (tiles * Lt * Lt > maxTileFloats) maxTileFloats = tiles * Lt * Lt;
        if (tiles > maxTiles) maxTiles = tiles;
        if (tiles * R * R > maxDist) maxDist = tiles * R * R;
    }
    for (int l = 0; l < kMaxLevels; l++) L->refSq[l] = nullptr;
    if (c->fused) {
        for (int l = 0; l < c->levels; l++) L->refSq[l] = (float*)b.take((size_t)L->tcx[l] * L->tcy[l] * 4);
        for (int i = 0; i < 2; i++) {
            L->work[0].lkSum[i] = b.image(L->tw, L->th, 4);
            L->work[0].lkDiff[i] = b.image(L->tw, L->th, 4);
        }
    }
    L->Ix = b.image(L->tw, L->th, 4);  // (fused: the derivative images of the kernel-parameter chain, made on the fuse stream)
    L->Iy = b.image(L->tw, L->th, 4);
    if (!c->fused) {
        L->warped = b.image(L->tw, L->th, 4);
        L->It = b.image(L->tw, L->th, 4);
        L->rawf = b.image(L->W, L->H, 4);
        L->refTiles = (float*)b.take(maxTileFloats * 4);
        L->movTiles = (float*)b.take(maxTileFloats * 4);
        L->cc = (float*)b.take(maxTileFloats * 4);
        L->boxX = (float*)b.take(maxTileFloats * 4);
        L->boxY = (float*)b.take(maxTileFloats * 4);
        L->sqsum = (float*)b.take(maxTiles * 4);
        L->dist = (float*)b.take(maxDist * 4);
    }
    if (c->preAlign) {
        const size_t pb = mfsr_preAlign_pyramid_bytes(L->tw, L->th);
        L->ref.prePyr = b.take(pb);
        L->mov[0].prePyr = b.take(pb);
        L->preWork = b.take(mfsr_preAlign_workspace_bytes(c->preAlignMaxAngle));
        L->work[0].preResult = (mfsr_prealign*)b.take(sizeof(mfsr_prealign));
    }
    // frame-batched alignment: frames 1 .. group-1 of a group get intermediates of their own
    L->nAlign = c->fused ? mfsr_burst_group_size(c) : 1;
    for (int q = 1; q < L->nAlign; q++) {
        FrameProducts& M = L->mov[q];
        AlignScratch& S = L->work[q];
        M.half = b.image(L->hw, L->hh, 12);
        for (int i = 0; i < nl; i++) M.pyr[i] = b.image(L->tw >> i, L->th >> i, 4);
        for (int l = 0; l < c->levels; l++) S.shifts[l] = b.image(L->tcx[l], L->tcy[l], 8);
        for (int i = 0; i < 2; i++) {
            S.lkSum[i] = b.image(L->tw, L->th, 4);
            S.lkDiff[i] = b.image(L->tw, L->th, 4);
        }
        if (c->preAlign) {
            M.prePyr = b.take(mfsr_preAlign_pyramid_bytes(L->tw, L->th));
            S.preResult = (mfsr_prealign*)b.take(sizeof(mfsr_prealign));
        }
    }
    for (int i = 0; i < c->uploadRing; i++) L->rawRing[i] = (uint16_t*)b.take((size_t)L->W * L->H * 2);
    if (c->uploadRing > 0)
        for (int i = 0; i < 2; i++) L->refRaw[i] = (uint16_t*)b.take((size_t)L->W * L->H * 2);
    // the erosion cannot run in place: one scratch mask per frame of a group, and only when the option is on
    if (c->maskErode > 0)
        for (int i = 0; i < mfsr_burst_group_size(c); i++) L->maskRaw[i] = b.image(L->hw, L->hh, 16);
    if (c->rawPacking != MFSR_PACK_NONE)
        for (int i = 0; i < c->uploadRing + 2; i++)
            L->stage[i] = (uint8_t*)b.take((size_t)mfsr_packed_row_bytes(c->rawPacking, L->W) * L->H);
    // ring slots beyond the first kRing (bursts of more than kRing frames): at the END, so that everything above keeps its place
    for (int i = kRing; i < ring_size(c); i++) {
        L->flowBuf[2 * i] = b.image(L->tw, L->th, 8);
        L->flowBuf[2 * i + 1] = b.image(L->tw, L->th, 8);
        L->maskBuf[i] = b.image(L->hw, L->hh, 16);
    }
    L->total = align_up(b.off, 256);
    return layout;
}

mfsr_tex2d as_tex(const Img& im)
{
    mfsr_tex2d t;
    t.ptr = im.ptr;
    t.pitch = im.pitch;
    t.width = im.w;
    t.height = im.h;
    return t;
}

}  // namespace

// The frames of one warp+fuse launch.  A group waits in one of three places of the burst: the filling group (pend), the host
// burst's second-to-last group (held), the burst hold (hold[]); every function that acts on a group takes it as an argument.
struct FuseGroup {
    int n;  // frames (the filling group: 0 .. group - 1 waiting)
    int slot[MFSR_MAX_FUSE_GROUP];
    const uint16_t* raw[MFSR_MAX_FUSE_GROUP];
    const Img* flow[MFSR_MAX_FUSE_GROUP];
    const Img* mask[MFSR_MAX_FUSE_GROUP];
    bool deferred[MFSR_MAX_FUSE_GROUP];  // not aligned yet: align_deferred aligns the group's waiting frames as one batch
    int isRef[MFSR_MAX_FUSE_GROUP];
    mfsr_float3 *imgOut, *totalWeights;
};

struct mfsr_burst {
    mfsr_burst(const mfsr_config& c, char* workspace) : cfg(c), L(make_layout(&c, workspace)) {}
    mfsr_config cfg;
    int cfa;            // cfg.cfa as the kernels' launch word (mfsr_pack_cfa), checked at create
    const Layout L;     // written by make_layout only
    FrameProducts ref;  // the current reference's products: L.ref, or what the caller of set_reference_impl supplied
    float taps[99];
    int ntaps;
    float tensorTaps[99];
    int ntensorTaps;
    const Img* flowCur;  // flow of the last add_frame (raw-pixel units)
    const Img* maskCur;  // certainty mask of the last add_frame
    mfsr_prealign* preCur;  // pre-alignment estimate of the last aligned frame (cfg.preAlign; device memory)
    bool haveRef;
    bool refStale;                      // `ref` names memory the burst does not own (process_joint's workspace): finish is
                                        // still valid, aligning another frame needs a new set_reference
    // frame grouping (cfg.pairFrames): aligned frames wait here until their group is complete, then the
    // group is fused in one pass over the accumulators; flush/finish fuses what is left of a group
    FuseGroup pend;
    // host bursts: the burst's second-to-last group, aligned and waiting with the last one (pend) for mfsr_burst_finish_host,
    // which fuses both band by band (heldHas: the entries of `held` are valid)
    FuseGroup held;
    bool heldHas;
    int group;  // frames per warp+fuse launch (mfsr_burst_group_size)
    // burst hold (mfsr_burst_hold_fuse): complete, aligned groups whose fuse waits for flush / finish / a full ring, where
    // two or more of them leave as ONE launch (mfsr_accumulateSuperResBurst); in arrival order, all on the same accumulators
    bool holdFuse;
    int nHold;
    FuseGroup hold[MFSR_MAX_BURST_FUSE / MFSR_MAX_FUSE_GROUP];
    int burstLaunches, burstGroups;  // burst launches since mfsr_burst_begin and the groups they fused (mfsr_burst_fuse_stats)
    int nFramesTimed;
    // mfsr_burst_begin: these accumulators are to be overwritten by the first fuse instead of zeroed
    struct Fresh {
        bool has;
        mfsr_float3 *imgOut, *totalWeights;
    } fresh;
    // ring + asynchronous fuse (cfg.asyncFuse)
    int frameCounter;
    hipStream_t fuseStream;             // high priority, non-blocking; null without asyncFuse
    int ring;                           // ring slots of this context (ring_size(cfg))
    hipEvent_t evAligned[kRingMax];     // recorded on the caller's stream when slot's flow/mask are complete
    hipEvent_t evFused[kRingMax];       // recorded on fuseStream when the fuse that read the slot is done
    // the reference products only the fuse and the finish read (kernel parameters, debayered fallback image) are made on
    // fuseStream, beside the alignment of the first group on the caller's stream: off the critical path of the burst
    hipEvent_t evRefStart, evRefDone;
    bool refOnFuse;                     // evRefDone is pending for consumers on other streams than fuseStream
    bool fusedOutstanding[kRingMax];    // evFused[slot] recorded and not yet waited for by the caller's stream
    const Img* slotFlow[kRingMax];      // which buffer of the slot's LK ping-pong pair holds the frame's final flow
    // host-frame bursts (cfg.uploadRing): copy stream, per-slot events, reference double buffer
    hipStream_t copyStream;
    hipStream_t downStream;                 // D2H of the finished image (mfsr_burst_finish_host), concurrent with the uploads
    hipEvent_t evFinished, evDown;          // finish kernel done (compute stream) / D2H done (down stream)
    bool downRecorded;
    hipEvent_t evBand[16];                  // host bursts: band i of the output image finished (mfsr_burst_finish_host)
    int framesSinceRef;                     // frames added since the last set_reference
    bool holdLastGroup;                     // host bursts: the group the burst's last frame completes waits for finish_host
    hipEvent_t evUp[kMaxUploadRing + 2];    // upload of the slot complete (copy stream); [ring..ring+1] = reference slots
    hipEvent_t evFree[kMaxUploadRing + 2];  // last consumer of the slot enqueued (compute / fuse stream)
    bool freeRecorded[kMaxUploadRing + 2];
    hipStream_t freeOn[kMaxUploadRing + 2]; // the stream evFree was recorded on
    int hostRowBytes;                       // row stride of the host frames (mfsr_burst_set_host_row_bytes); 0 = dense
    // rendered output (mfsr_burst_set_render): the out16 arguments of the finishes are bytes of render.format
    bool renderOn;
    mfsr_render render;
    // sharpening inside the finish (mfsr_burst_set_sharpen)
    bool sharpenOn;
    mfsr_sharpen sharpen;
    int sharpenedFinishes;  // launches of mfsr_finishSharpened since mfsr_burst_begin (mfsr_burst_debug_sharpened)
    // merge-aware denoise inside the finish (mfsr_burst_set_denoise); never on together with sharpenOn
    bool denoiseOn;
    mfsr_denoise denoise;
    int denoisedFinishes;   // launches of mfsr_finishDenoised since mfsr_burst_begin (mfsr_burst_debug_denoised)
    int robustGroupLaunches;  // launches of mfsr_robustnessMaskGroup since mfsr_burst_begin (mfsr_burst_debug_robust_group)
    // The finish inside the burst launch (mfsr_accumulateSuperResBurstFinish): mfsr_burst_finish sets finishOut16 before it
    // flushes when the hold's launch is the burst's last fuse and the plain whole-frame uint16_t image is all it was asked for;
    // drain_waiting then issues the finishing launch and sets finishTaken, or launches as ever where the entry refuses.
    uint16_t* finishOut16;
    bool finishTaken;
    int fusedFinishes;  // finishes taken that way since mfsr_burst_begin (mfsr_burst_debug_finish_fused)
    // host staging of mfsr_burst_auto_render: the downloaded table and the tone table on its way to the device
    std::vector<uint64_t> autoStats;
    std::vector<float> autoLut;
    // local tone mapping in the finish (mfsr_burst_set_local_tone): the installed grid (the caller's device
    // memory) and the host staging of mfsr_burst_local_tone; never on together with a stencil or a two-plane format
    bool localToneOn;
    mfsr_local_tone localTone;
    const float* localToneGrid;
    std::vector<uint64_t> toneStats;
    std::vector<float> toneGrid;
    // the finish chain (mfsr_burst_set_finish_chain): denoise, sharpen and local tone in one launch, to any
    // format; never installed together with sharpenOn, denoiseOn or localToneOn
    bool chainOn;
    mfsr_finish_chain chain;
    const float* chainGrid;  // the caller's device memory, or null without the chain's local tone
    int chainReach;          // R_d + R_s of the installed chain
    int chainedFinishes;     // launches of mfsr_finishChain since mfsr_burst_begin (mfsr_burst_debug_chained)
    int geometryFinishes;    // launches of mfsr_finishGeometry since mfsr_burst_begin (mfsr_burst_debug_geometry)
    // a host burst captured into a graph (host_epoch): the capture the per-slot events above were recorded in (0 = none, the
    // eager launch sequence), and the event that forks the copy and the download stream off the caller's when that changes
    unsigned long long hostEpoch;
    hipEvent_t evEpoch;
    // cfg.rawPacking: a slot's upload lands in L.stage[slot]; the compute stream unpacks it into the slot
    hipEvent_t evUnp[kMaxUploadRing + 2];   // recorded on the compute stream after an unpack launch whose first slot this is
    hipEvent_t unpDone[kMaxUploadRing + 2]; // the event (one of evUnp) after the launch that last read the slot's staging; or null
    int unpQ[kMaxUploadRing + 2], nUnp;     // slots uploaded and not unpacked yet, in the order of their uploads
    // mfsr_burst_prefetch_host: frames whose upload is already enqueued, in order; consumed by add_frame_host
    struct Prefetched {
        const uint16_t* host;
        int slot;
    } prefetched[kMaxUploadRing];
    int nPrefetched, prefetchHead;
    bool upPending;                         // uploads were enqueued that the compute stream has not been made to wait for yet
    int upPendingSlot;                      // ... the LAST of them (the copy stream is in order: its event covers the earlier ones)
    int refSlot;                            // upload slot of the current host reference (-1: none / released)
    bool hostBusy;                          // this host burst was enqueued before the previous one's download had finished
    int upCounter, refCounter;
    const uint16_t* refHost;                // host pointer of the current reference and its device copy
    const uint16_t* refDev;
    std::vector<float> jointHost;  // host staging of the joint mode's design matrix / pointer table (must outlive the copies)
    // zoom window (mfsr_burst_set_window): the HR rectangle the fuse / finish work on, window-sized buffers; `win` is in
    // effect, `winNext` is adopted by the next set_reference (on = false: the whole frame, whole-frame buffers)
    struct Window {
        bool on = false;
        int x0 = 0, y0 = 0, w = 0, h = 0;
    } win, winNext;
    // optional per-launch timing of the accumulate kernel (bench.py roofline leg)
    bool timing;
    int nEvents;
    hipEvent_t evStart[kMaxTimedLaunches], evStop[kMaxTimedLaunches];
    unsigned char evLaunches[kMaxTimedLaunches];  // launches an event pair stands for: 1, or the groups of a burst launch
    // which branches the driver took since mfsr_burst_begin (mfsr_burst_debug_paths): host-side counters only
    int32_t paths[MFSR_PATH_COUNT];
};

#define TRY(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != MFSR_OK) return rc_; \
    } while (0)

static int flush_pending(mfsr_burst* b, mfsr_stream_t stream, bool materializeFresh = true);

// extent of the burst's output (the window or the whole HR grid) and the bytes of one accumulator plane-set of it
static int out_w(const mfsr_burst* b) { return b->win.on ? b->win.w : b->L.hrW; }
static int out_h(const mfsr_burst* b) { return b->win.on ? b->win.h : b->L.hrH; }
static size_t acc_bytes(const mfsr_burst* b) { return (size_t)12 * out_w(b) * out_h(b); }

// the config's levels as the kernels take them
static mfsr_float3 cfg_white(const mfsr_config& c) { return {c.white[0], c.white[1], c.white[2]}; }
static mfsr_float3 cfg_black(const mfsr_config& c) { return {c.black[0], c.black[1], c.black[2]}; }

// the certainty masks and the flows of an aligned group, frame i at masks[i] / flows[i]
static void group_tables(const FuseGroup& g, mfsr_tex2d* masks, mfsr_tex2d* flows)
{
    for (int i = 0; i < g.n; i++) {
        masks[i] = as_tex(*g.mask[i]);
        flows[i] = as_tex(*g.flow[i]);
    }
}

// stage G of an aligned group onto its accumulators, output rows [r0, r1) of the burst's output (the window's rows when one is
// set; the group's pointers are the accumulators' first pixel either way)
static int fuse_group(mfsr_burst* b, const FuseGroup& g, int fresh, int r0, int r1, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const mfsr_float3 white = cfg_white(c), black = cfg_black(c);
    mfsr_tex2d maskTex[MFSR_MAX_FUSE_GROUP], flows[MFSR_MAX_FUSE_GROUP];
    group_tables(g, maskTex, flows);
    const mfsr_float4* masks[MFSR_MAX_FUSE_GROUP];
    for (int i = 0; i < g.n; i++) masks[i] = (const mfsr_float4*)maskTex[i].ptr;
    const int maskPitch = maskTex[0].pitch;
    if (!b->win.on)
        return mfsr_cfa::accumulateSuperResFullRows(b->cfa, g.n, g.raw, g.imgOut, g.totalWeights, masks, as_tex(L.kparam4), flows, white, black,
                                               L.W, L.H, c.scale, 12 * L.hrW, maskPitch, fresh, r0, r1, stream);
    const int pitch = 12 * b->win.w;
    const size_t off = (size_t)r0 * pitch;
    return mfsr_cfa::accumulateSuperResFullWindow(b->cfa, g.n, g.raw, (mfsr_float3*)((char*)g.imgOut + off),
                                             (mfsr_float3*)((char*)g.totalWeights + off), masks, as_tex(L.kparam4), flows, white, black, L.W,
                                             L.H, c.scale, pitch, maskPitch, fresh, b->win.x0, b->win.y0 + r0, b->win.w, r1 - r0, stream);
}

extern "C" int mfsr_config_default(mfsr_config* cfg, int width, int height, int frames, int scale, int mono)
{
    MFSR_REQUIRE(cfg != nullptr);
    memset(cfg, 0, sizeof(*cfg));
    cfg->width = width;
    cfg->height = height;
    cfg->frames = frames;
    cfg->reference = 0;
    cfg->scale = scale;
    cfg->mono = mono;
    if (mono) {
        cfg->cfa[0] = cfg->cfa[1] = cfg->cfa[2] = cfg->cfa[3] = MFSR_GREEN;
    } else {
        cfg->cfa[0] = MFSR_RED;
        cfg->cfa[1] = MFSR_GREEN;
        cfg->cfa[2] = MFSR_GREEN;
        cfg->cfa[3] = MFSR_BLUE;
    }
    // 12-bit sensor, black level 256 (SURVEY.md section 8d synthetic-input recipe)
    for (int i = 0; i < 3; i++) {
        cfg->black[i] = 256.0f;
        cfg->white[i] = 4095.0f - 256.0f;
    }
    cfg->maxVal = 4095.0f;
    cfg->levels = 2;
    cfg->levelFactor[0] = 2;
    cfg->levelFactor[1] = 1;
    cfg->tileSize[0] = 32;
    cfg->tileSize[1] = 32;
    cfg->maxShift[0] = 4;
    cfg->maxShift[1] = 4;
    cfg->minimumThreshold = 0.0f;
    cfg->sigmaTracking = 0.5f;  // SigmaDebayerTracking, test_opencv/main.cpp:1868
    cfg->lkIterations = 3;
    cfg->lkHalfWindow = 3;
    cfg->lkMinDet = 1e-4f;
    cfg->alpha = 1e-4f;
    cfg->beta = 1e-6f;
    cfg->thresholdM = 1.0f;
    cfg->sigmaTensor = 1.0f;
    cfg->Dth = 0.005f;
    cfg->Dtr = 0.05f;
    cfg->kDetail = 0.3f;
    cfg->kDenoise = 2.0f;
    cfg->kStretch = 2.0f;
    cfg->kShrink = 2.0f;
    cfg->weightThreshold = 1e-3f;
    cfg->applyGamma = 0;
    cfg->fused = 1;
    cfg->pairFrames = 1;
    cfg->preAlign = 0;   // opt-in: bursts with rotations / shifts beyond the tile tracker's reach (the bundled "city" burst)
    cfg->preAlignMaxAngle = 20.0f;
    cfg->asyncFuse = 0;  // 1: warp+fuse launches on a burst-owned stream beside the alignment of the next group.  It paid +5 % in
                         // round 2; since the fuse kernel keeps four 128-VGPR workgroups per CU (round 3) nothing of the alignment
                         // gets onto a CU beside it -- the two streams alternate -- and the fork / join events cost more than
                         // the overlap returns: 5.97 ms per 4K x 16 burst on one stream against 6.03 on two (interleaved A/B,
                         // profiles/r04_async_fuse_ab.txt).  Off by default since round 4; bit-identical either way.
    return MFSR_OK;
}

extern "C" size_t mfsr_burst_workspace_bytes(const mfsr_config* cfg)
{
    if (validate(cfg) != MFSR_OK) return 0;
    return make_layout(cfg, nullptr).total;
}

extern "C" size_t mfsr_burst_accumulator_bytes(const mfsr_config* cfg)
{
    if (!cfg || cfg->width <= 0 || cfg->height <= 0 || cfg->scale <= 0) return 0;
    return (size_t)12 * cfg->scale * cfg->width * (size_t)cfg->scale * cfg->height;
}

extern "C" int mfsr_burst_create(mfsr_burst** out, const mfsr_config* cfg, void* workspace, size_t workspaceBytes)
{
    MFSR_REQUIRE(out != nullptr && workspace != nullptr);
    TRY(validate(cfg));
    int cfa = 0;
    TRY(mfsr_pack_cfa(cfg->cfa, &cfa));
    if (mfsr_device_count() <= 0) {
        fprintf(stderr, "mfsr: no HIP device available (there is no CPU fallback)\n");
        return MFSR_E_NODEVICE;
    }
    MFSR_REQUIRE(((uintptr_t)workspace & 255) == 0);
    mfsr_burst* b = new (std::nothrow) mfsr_burst(*cfg, (char*)workspace);
    MFSR_REQUIRE(b != nullptr);
    if (b->L.total > workspaceBytes) {
        fprintf(stderr, "mfsr: workspace too small: need %zu bytes, got %zu\n", b->L.total, workspaceBytes);
        delete b;
        return MFSR_E_WORKSPACE;
    }
    b->cfa = cfa;
    b->ntaps = mfsr_gaussin_filter_1D(cfg->sigmaTracking, b->taps);
    b->ntensorTaps = mfsr_gaussin_filter_1D(cfg->sigmaTensor, b->tensorTaps);
    b->flowCur = &b->L.flowBuf[0];
    b->maskCur = &b->L.maskBuf[0];
    b->preCur = b->L.work[0].preResult;
    b->ref = b->L.ref;
    b->pend.n = 0;
    b->group = mfsr_burst_group_size(&b->cfg);
    b->ring = ring_size(&b->cfg);
    b->holdFuse = false;
    b->nHold = 0;
    b->burstLaunches = b->burstGroups = 0;
    b->fresh.has = false;
    b->nFramesTimed = 0;
    b->timing = false;
    b->nEvents = 0;
    memset(b->evStart, 0, sizeof(b->evStart));
    memset(b->evStop, 0, sizeof(b->evStop));
    b->frameCounter = 0;
    b->fuseStream = nullptr;
    b->evRefStart = b->evRefDone = nullptr;
    b->refOnFuse = false;
    for (int i = 0; i < kRingMax; i++) {
        b->evAligned[i] = b->evFused[i] = nullptr;
        b->fusedOutstanding[i] = false;
        b->slotFlow[i] = nullptr;
    }
    if (cfg->asyncFuse) {
        int lo = 0, hi = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        // MFSR_FUSE_PRIO=low|normal (A/B): the fuse stream's priority against the caller's (default: high)
        static const int prioMode = [] {
            const char* v = getenv("MFSR_FUSE_PRIO");
            return !v ? 0 : (v[0] == 'l' ? 1 : (v[0] == 'n' ? 2 : 0));
        }();
        const int prio = prioMode == 1 ? lo : (prioMode == 2 ? (lo + hi) / 2 : hi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&b->fuseStream, hipStreamNonBlocking, prio);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evRefStart, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evRefDone, hipEventDisableTiming);
        for (int i = 0; i < b->ring && e == hipSuccess; i++) {
            e = hipEventCreateWithFlags(&b->evAligned[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evFused[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) {
            mfsr_burst_destroy(b);
            return MFSR_E_NODEVICE;
        }
    }
    b->copyStream = nullptr;
    b->downStream = nullptr;
    b->evFinished = b->evDown = nullptr;
    b->downRecorded = false;
    b->upCounter = b->refCounter = 0;
    for (int i = 0; i < 16; i++) b->evBand[i] = nullptr;
    b->framesSinceRef = 0;
    b->holdLastGroup = false;
    b->heldHas = false;
    b->held.n = 0;
    b->refHost = b->refDev = nullptr;
    b->refSlot = -1;
    b->hostBusy = false;
    b->upPending = false;
    b->upPendingSlot = -1;
    b->nPrefetched = b->prefetchHead = 0;
    for (int i = 0; i < kMaxUploadRing + 2; i++) {
        b->evUp[i] = b->evFree[i] = b->evUnp[i] = b->unpDone[i] = nullptr;
        b->freeRecorded[i] = false;
        b->freeOn[i] = nullptr;
    }
    b->hostRowBytes = 0;
    b->renderOn = false;
    b->sharpenOn = false;
    b->sharpenedFinishes = 0;
    b->denoiseOn = false;
    b->denoisedFinishes = 0;
    b->localToneOn = false;
    b->localToneGrid = nullptr;
    b->chainOn = false;
    b->chainGrid = nullptr;
    b->chainReach = 0;
    b->chainedFinishes = 0;
    b->geometryFinishes = 0;
    b->robustGroupLaunches = 0;
    b->finishOut16 = nullptr;
    b->finishTaken = false;
    b->fusedFinishes = 0;
    b->nUnp = 0;
    b->hostEpoch = 0;
    b->evEpoch = nullptr;
    if (cfg->uploadRing > 0) {
        hipError_t e = hipStreamCreateWithFlags(&b->copyStream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->downStream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evFinished, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evDown, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evEpoch, hipEventDisableTiming);
        for (int i = 0; i < cfg->uploadRing + 2 && e == hipSuccess; i++) {
            e = hipEventCreateWithFlags(&b->evUp[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evFree[i], hipEventDisableTiming);
            if (e == hipSuccess && cfg->rawPacking != MFSR_PACK_NONE) e = hipEventCreateWithFlags(&b->evUnp[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) {
            mfsr_burst_destroy(b);
            return MFSR_E_NODEVICE;
        }
    }
    b->haveRef = false;
    b->refStale = false;
    memset(b->paths, 0, sizeof(b->paths));
    *out = b;
    return MFSR_OK;
}

extern "C" void mfsr_burst_destroy(mfsr_burst* b)
{
    if (!b) return;
    for (int i = 0; i < kMaxTimedLaunches; i++) {
        if (b->evStart[i]) (void)hipEventDestroy(b->evStart[i]);
        if (b->evStop[i]) (void)hipEventDestroy(b->evStop[i]);
    }
    if (b->fuseStream) (void)hipStreamSynchronize(b->fuseStream);
    for (int i = 0; i < kRingMax; i++) {
        if (b->evAligned[i]) (void)hipEventDestroy(b->evAligned[i]);
        if (b->evFused[i]) (void)hipEventDestroy(b->evFused[i]);
    }
    if (b->evRefStart) (void)hipEventDestroy(b->evRefStart);
    if (b->evRefDone) (void)hipEventDestroy(b->evRefDone);
    if (b->fuseStream) (void)hipStreamDestroy(b->fuseStream);
    if (b->copyStream) (void)hipStreamSynchronize(b->copyStream);
    if (b->downStream) (void)hipStreamSynchronize(b->downStream);
    if (b->evFinished) (void)hipEventDestroy(b->evFinished);
    if (b->evDown) (void)hipEventDestroy(b->evDown);
    if (b->evEpoch) (void)hipEventDestroy(b->evEpoch);
    for (int i = 0; i < 16; i++)
        if (b->evBand[i]) (void)hipEventDestroy(b->evBand[i]);
    if (b->downStream) (void)hipStreamDestroy(b->downStream);
    for (int i = 0; i < kMaxUploadRing + 2; i++) {
        if (b->evUp[i]) (void)hipEventDestroy(b->evUp[i]);
        if (b->evFree[i]) (void)hipEventDestroy(b->evFree[i]);
        if (b->evUnp[i]) (void)hipEventDestroy(b->evUnp[i]);
    }
    if (b->copyStream) (void)hipStreamDestroy(b->copyStream);
    delete b;
}

// Per-launch timing of the warp+fuse (accumulate) kernel with HIP events recorded
// on the caller's stream around each launch.  enable != 0 starts a fresh series.
extern "C" int mfsr_burst_timing(mfsr_burst* b, int enable)
{
    MFSR_REQUIRE(b != nullptr);
    b->timing = enable != 0;
    b->nEvents = 0;
    b->nFramesTimed = 0;
    return MFSR_OK;
}

// Synchronises with the recorded events and returns the summed kernel time and
// the number of timed launches since mfsr_burst_timing(b, 1).
extern "C" int mfsr_burst_timing_read(mfsr_burst* b, double* totalMs, int* launches, int* frames)
{
    MFSR_REQUIRE(b && totalMs && launches && frames);
    double total = 0;
    int nLaunches = 0;
    for (int i = 0; i < b->nEvents; i++) {
        MFSR_HIP_TRY(hipEventSynchronize(b->evStop[i]));
        float ms = 0;
        MFSR_HIP_TRY(hipEventElapsedTime(&ms, b->evStart[i], b->evStop[i]));
        total += ms;
        nLaunches += b->evLaunches[i];
    }
    *totalMs = total;
    *launches = nLaunches;
    *frames = b->nFramesTimed;
    b->nEvents = 0;
    b->nFramesTimed = 0;
    return MFSR_OK;
}

// host-frame bursts: `stream` is about to read raw frames the copy stream uploads -- wait for the last upload enqueued so far
// (cfg.rawPacking: the frames then arrived packed, in the slots' staging buffers -- `stream` also unpacks them into the slots)
static int unpack_uploaded(mfsr_burst* b, int lastSlot, mfsr_stream_t stream);
static int wait_uploads(mfsr_burst* b, mfsr_stream_t stream)
{
    if (b->upPending) {
        MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evUp[b->upPendingSlot], 0));
        b->upPending = false;
        if (b->nUnp > 0) TRY(unpack_uploaded(b, b->upPendingSlot, stream));
    }
    return MFSR_OK;
}

// the last consumer of upload slot `us` has been enqueued on `stream`: whoever writes the slot next waits for it
static int record_free(mfsr_burst* b, int us, mfsr_stream_t stream)
{
    MFSR_HIP_TRY(hipEventRecord(b->evFree[us], mfsr_s(stream)));
    b->freeRecorded[us] = true;
    b->freeOn[us] = mfsr_s(stream);
    return MFSR_OK;
}

// cfg.rawPacking: `stream` has waited for the upload of lastSlot, so every upload queued up to it has landed (the copy stream is
// in order).  ONE mfsr_unpackRaw launch widens them from their staging buffers into their slots.  The slots' previous frames may
// still be read on another stream (the fuse stream of cfg.asyncFuse): the launch waits for each slot's evFree -- the wait the copy
// stream makes when it writes the slots itself.  The staging buffers may be refilled after the launch: the event recorded here.
static int unpack_uploaded(mfsr_burst* b, int lastSlot, mfsr_stream_t stream)
{
    const Layout& L = b->L;
    int n = 0;
    while (n < b->nUnp && b->unpQ[n] != lastSlot) n++;
    if (n == b->nUnp) return MFSR_OK;  // (unpacked already, with a later upload)
    n++;
    const uint8_t* packed[kMaxUploadRing + 2];
    uint16_t* frames[kMaxUploadRing + 2];
    for (int i = 0; i < n; i++) {
        const int us = b->unpQ[i];
        packed[i] = L.stage[us];
        frames[i] = us < b->cfg.uploadRing ? L.rawRing[us] : L.refRaw[us - b->cfg.uploadRing];
        if (b->freeRecorded[us]) {
            if (b->freeOn[us] != mfsr_s(stream)) MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evFree[us], 0));
            b->freeRecorded[us] = false;
        }
    }
    static_assert(kMaxUploadRing + 2 <= kRawMaxFrames, "one launch takes every upload slot");
    TRY(mfsr_unpackRaw(n, packed, mfsr_packed_row_bytes(b->cfg.rawPacking, L.W), b->cfg.rawPacking, frames, 2 * L.W, L.W, L.H, stream));
    hipEvent_t done = b->evUnp[b->unpQ[0]];
    MFSR_HIP_TRY(hipEventRecord(done, mfsr_s(stream)));
    for (int i = 0; i < n; i++) b->unpDone[b->unpQ[i]] = done;
    for (int i = n; i < b->nUnp; i++) b->unpQ[i - n] = b->unpQ[i];
    b->nUnp -= n;
    return MFSR_OK;
}

// A1 + tracking pyramid for one frame (shared by reference and moved frames)
static int prepare_frame(mfsr_burst* b, const uint16_t* raw, const FrameProducts& f, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const Img& half = f.half;
    const Img* pyr = f.pyr;
    const float maxValEff = c.mono ? 2.0f * c.maxVal : c.maxVal;  // mono: 4 "greens" x 0.5 -> mean of the quad
    const int nlev = ilog2(L.maxFactor) + 1;
    if (c.fused && !c.mono && b->ntaps / 2 <= 8 && L.tw == L.hw && L.th == L.hh) {
        // A1 + luma + prefilter + first pyramid level in one launch (bit-identical to the chain below)
        const mfsr_prepare_frame pf = {raw, (mfsr_float3*)half.ptr, (float*)pyr[0].ptr, nlev > 1 ? (float*)pyr[1].ptr : nullptr};
        TRY(mfsr_cfa::prepareFrames(b->cfa, 1, &pf, half.pitch, maxValEff, L.hw, L.hh, pyr[0].pitch, nlev > 1 ? pyr[1].pitch : 0, b->taps,
                                    b->ntaps, stream, false));
        b->paths[MFSR_PATH_PREPARE_FUSED]++;
        for (int i = 2; i < nlev; i++)
            TRY(mfsr_downsample2x((const float*)pyr[i - 1].ptr, pyr[i - 1].pitch, (float*)pyr[i].ptr, pyr[i].pitch, pyr[i].w,
                                  pyr[i].h, stream));
        return MFSR_OK;
    }
    b->paths[MFSR_PATH_PREPARE_CHAIN]++;
    TRY(mfsr_cfa::deBayersSubSample3(b->cfa, raw, (mfsr_float3*)half.ptr, maxValEff, L.hw, L.hh, half.pitch, stream));
    if (c.mono)
        TRY(mfsr_u16ToFloat(raw, (float*)L.tmpA.ptr, L.tmpA.pitch, L.W, L.H, 1.0f / c.maxVal, stream));
    else
        TRY(mfsr_rgbToGray((const mfsr_float3*)half.ptr, half.pitch, (float*)L.tmpA.ptr, L.tmpA.pitch, L.tw, L.th, stream));
    TRY(mfsr_separableFilter((const float*)L.tmpA.ptr, L.tmpA.pitch, (float*)L.tmpB.ptr, (float*)pyr[0].ptr, pyr[0].pitch,
                             L.tw, L.th, 1, b->taps, b->ntaps, stream));
    const int nl = ilog2(L.maxFactor) + 1;
    for (int i = 1; i < nl; i++)
        TRY(mfsr_downsample2x((const float*)pyr[i - 1].ptr, pyr[i - 1].pitch, (float*)pyr[i].ptr, pyr[i].pitch, pyr[i].w,
                              pyr[i].h, stream));
    return MFSR_OK;
}

// reference products.  [hrRow0, hrRow1) = the HR rows whose fuse / finish will read the kernel parameters and the fallback image
// (the whole grid for a single-GPU burst; a stripe for a rank of a multi-GPU burst: those two products are then made for
// the rows the stripe reads plus the halo their stencils need -- every kernel below works on a row window of the images,
// so the rows it makes are the bits the whole-image run makes)
// prepared: the frame's products, made by the caller (frame streams, joint mode) -- null: made here, into L.ref
static int set_reference_impl(mfsr_burst* b, const uint16_t* rawRef, int hrRow0, int hrRow1, mfsr_stream_t stream,
                              const FrameProducts* prepared = nullptr)
{
    MFSR_REQUIRE(b && rawRef);
    TRY(flush_pending(b, stream, false));  // a frame still waiting belongs to the previous reference
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    MFSR_REQUIRE(hrRow0 >= 0 && hrRow1 > hrRow0 && hrRow1 <= L.hrH);
    // a zoom window set since the last reference takes effect here: the products below are made for its rows
    MFSR_REQUIRE(!b->winNext.on || (hrRow0 == 0 && hrRow1 == L.hrH));  // (a window is not combined with row stripes)
    b->win = b->winNext;
    if (b->win.on) {
        hrRow0 = b->win.y0;
        hrRow1 = b->win.y0 + b->win.h;
    }
    const bool whole = (hrRow0 == 0 && hrRow1 == L.hrH) || !c.fused;  // (the unfused chain always makes whole images)
    TRY(wait_uploads(b, stream));
    b->ref = prepared ? *prepared : L.ref;
    const FrameProducts& R = b->ref;
    if (!prepared) TRY(prepare_frame(b, rawRef, R, stream));
    const bool refFused = c.fused && mfsr_reference_fused();  // (mfsr_set_reference_fused(0): the launches this replaced, A/B)
    // MFSR_REF_FUSED_PARTS: which parts of the fused setup run, for A/B of one part (1 kernel field, 2 tile sums, 4 ring debayer)
    static const int refParts = mfsr_env_int("MFSR_REF_FUSED_PARTS", 7);
    const bool fusedField = refFused && (refParts & 1), fusedSums = refFused && (refParts & 2), fusedRing = refFused && (refParts & 4);
    if (fusedSums) {
        mfsr_tex2d lv[kMaxLevels];
        for (int l = 0; l < c.levels; l++) lv[l] = as_tex(R.pyr[ilog2(c.levelFactor[l])]);
        TRY(mfsr_tileSquaredSumsLevels(c.levels, lv, L.refSq, c.maxShift, c.tileSize, L.tcx, L.tcy, stream));
    } else if (c.fused)
        for (int l = 0; l < c.levels; l++) {
            const Img& ref = R.pyr[ilog2(c.levelFactor[l])];
            TRY(mfsr_tileSquaredSums((const float*)ref.ptr, L.refSq[l], ref.w, ref.h, ref.pitch, c.maxShift[l], c.tileSize[l],
                                     L.tcx[l], L.tcy[l], stream));
        }

    if (c.preAlign) {
        TRY(mfsr_preAlign_init(L.preWork, c.preAlignMaxAngle, stream));
        if (!prepared) TRY(mfsr_preAlignPyramid((const float*)R.pyr[0].ptr, L.tw, L.th, R.pyr[0].pitch, R.prePyr, stream));
    }

    // What follows is read by the fuse and the finish only, not by the alignment: with cfg.asyncFuse it runs on the burst's fuse
    // stream (after everything the caller's stream has enqueued so far: the previous burst's finish reads the same images),
    // beside the alignment of the first group -- 0.2 ms off the burst's critical path, on which the GPU is otherwise
    // half empty.  MFSR_REF_OVERLAP=0: on the caller's stream (A/B).
    static const bool refOverlap = !mfsr_env_is0("MFSR_REF_OVERLAP");
    mfsr_stream_t es = stream;
    b->refOnFuse = false;
    if (refOverlap && b->fuseStream && c.fused) {
        MFSR_HIP_TRY(hipEventRecord(b->evRefStart, mfsr_s(stream)));
        MFSR_HIP_TRY(hipStreamWaitEvent(b->fuseStream, b->evRefStart, 0));
        es = (mfsr_stream_t)b->fuseStream;
    }
    // E: kernel shape field from the reference tracking image
    // E1 + E2 run once per burst on an LR-sized image, and E3 turns their result into the kernel ORIENTATION through an
    // eigen-decomposition that is ill-conditioned wherever the tensor is nearly isotropic (k1 != k2 even there,
    // kernel.cu:766-772): a tensor that differs in its last bits (mfsr_structureTensorFused reads the texels directly
    // instead of blending them with the ~1e-7 weights an exact-float bilinear fetch at a texel centre has) moves the tap
    // exponents by up to 0.5 there, i.e. the accumulators by 1e-3 relative -- measured, tools/parity_audit.py.  So the
    // field is made with the arithmetic of the bit-exact kernel chain (field_math.hpp): in one launch by
    // mfsr_kernelParamField, which keeps the five intermediates in LDS, or, where that kernel declines (more than 11
    // tensor taps, an image below one of its tiles, mfsr_set_reference_fused(0), cfg.fused = 0), by the chain itself.
    {
        // field rows the fuse of HR rows [hrRow0, hrRow1) samples: floor((Y + .5) * th / hrH - .5) and the next one; the
        // smoothing reads taps / 2 more on either side (clamped at the IMAGE border only: the window carries that halo)
        int f0 = 0, f1 = L.th;
        if (!whole) {
            const int per = L.hrH / L.th, halo = b->ntensorTaps / 2 + 1;
            f0 = hrRow0 / per - 1 - halo;
            f1 = (hrRow1 + per - 1) / per + 1 + halo;
            f0 = f0 < 0 ? 0 : f0;
            f1 = f1 > L.th ? L.th : f1;
        }
        const int fr = f1 - f0;
        int rcField = MFSR_E_UNSUPPORTED;
        if (fusedField) {
            rcField = mfsr_kernelParamField(as_tex(R.pyr[0]), as_tex(L.kparam4), f0, fr, b->tensorTaps, b->ntensorTaps, c.Dth, c.Dtr,
                                            c.kDetail, c.kDenoise, c.kStretch, c.kShrink, es);
            if (rcField != MFSR_E_UNSUPPORTED) TRY(rcField);
        }
        if (rcField == MFSR_OK) {
            b->paths[MFSR_PATH_REF_FIELD_FUSED]++;
        } else {
            const Img& ix = L.Ix;
            const Img& iy = L.Iy;
            auto rows = [&](const Img& im) { return (char*)im.ptr + (size_t)f0 * im.pitch; };
            TRY(mfsr_ComputeDerivatives2Rows(L.tw, L.th, ix.pitch, (float*)ix.ptr, (float*)iy.ptr, as_tex(R.pyr[0]), f0, fr, es));
            TRY(mfsr_ComputeStructureTensor((const float*)rows(ix), (const float*)rows(iy), (mfsr_float3*)rows(L.tensor), L.tw, fr,
                                            ix.pitch, L.tensor.pitch, es));
            TRY(mfsr_separableFilter((const float*)rows(L.tensor), L.tensor.pitch, (float*)rows(L.tensorTmp),
                                     (float*)rows(L.tensorSm), L.tensorSm.pitch, L.tw, fr, 3, b->tensorTaps, b->ntensorTaps, es));
            TRY(mfsr_ComputeKernelParam((mfsr_float3*)rows(L.tensorSm), L.tw, fr, L.tensorSm.pitch, c.Dth, c.Dtr, c.kDetail,
                                        c.kDenoise, c.kStretch, c.kShrink, es));
            TRY(mfsr_float3ToFloat4((const mfsr_float3*)rows(L.tensorSm), L.tensorSm.pitch, (mfsr_float4*)rows(L.kparam4),
                                    L.kparam4.pitch, L.tw, fr, es));
        }
    }

    // A2 + A3: debayered reference = fallback image of ApplyWeighting (finish resamples it bilinearly: raw rows Y / s +- 1;
    // the row window starts on an even row -- the CFA phase -- and carries the 3-row stencil halo plus the 2-row ring the
    // kernels leave untouched at a window edge)
    const mfsr_float3 bp = cfg_black(c);
    const mfsr_float3 sc = {1.0f / c.white[0], 1.0f / c.white[1], 1.0f / c.white[2]};
    int r0 = 0, r1 = L.H;
    if (!whole) {
        r0 = (hrRow0 / c.scale - 8) & ~1;
        r1 = ((hrRow1 + c.scale - 1) / c.scale + 8 + 1) & ~1;
        r0 = r0 < 0 ? 0 : r0;
        r1 = r1 > L.H ? L.H : r1;
    }
    char* fb = (char*)L.fallback.ptr + (size_t)r0 * L.fallback.pitch;
    // (the debayer kernels leave the 2-pixel ring of their image untouched: mfsr_deBayerFusedRing stores its zeros itself, the
    // others take them from a cleared image.  The clear also zeroed the pitch padding behind each row; without it the padding
    // keeps what the workspace held.  Nothing reads it: every consumer of the fallback image addresses pixels below L.W.)
    if (!fusedRing) MFSR_HIP_TRY(hipMemsetAsync(fb, 0, (size_t)L.fallback.pitch * (r1 - r0), mfsr_s(es)));
    if (c.fused) {
        if (fusedRing) {
            const mfsr_tex2d fbt = {fb, L.fallback.pitch, L.W, r1 - r0};
            TRY(mfsr_cfa::deBayerFusedRing(b->cfa, rawRef + (size_t)r0 * L.W, fbt, bp, sc, es));
        } else
            TRY(mfsr_cfa::deBayerFused(b->cfa, rawRef + (size_t)r0 * L.W, (mfsr_float3*)fb, L.fallback.pitch, L.W, r1 - r0, bp, sc, es));
        if (es != stream) {
            MFSR_HIP_TRY(hipEventRecord(b->evRefDone, b->fuseStream));
            b->refOnFuse = true;
        }
    } else {
        TRY(mfsr_u16ToFloat(rawRef, (float*)L.rawf.ptr, L.rawf.pitch, L.W, L.H, 1.0f, stream));
        TRY(mfsr_cfa::deBayerGreenKernel(b->cfa, L.W, L.H, (const float*)L.rawf.ptr, L.rawf.pitch, (mfsr_float3*)L.fallback.ptr,
                                    L.fallback.pitch, bp, sc, stream));
        TRY(mfsr_cfa::deBayerRedBlueKernel(b->cfa, L.W, L.H, (const float*)L.rawf.ptr, L.rawf.pitch, (mfsr_float3*)L.fallback.ptr,
                                      L.fallback.pitch, bp, sc, stream));
    }
    b->haveRef = true;
    b->refStale = false;
    b->framesSinceRef = 0;
    b->holdLastGroup = false;  // (set again by every mfsr_burst_add_frame_host)
    return MFSR_OK;
}

extern "C" int mfsr_burst_set_reference(mfsr_burst* b, const uint16_t* rawRef, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b != nullptr);
    return set_reference_impl(b, rawRef, 0, b->L.hrH, stream);
}

extern "C" int mfsr_burst_set_reference_rows(mfsr_burst* b, const uint16_t* rawRef, int hrRow0, int hrRow1, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b != nullptr);
    return set_reference_impl(b, rawRef, hrRow0, hrRow1, stream);
}

// ---- zoom windows ---------------------------------------------------------------------------------------------------------
extern "C" int mfsr_window_check(const mfsr_config* cfg, int x0, int y0, int w, int h)
{
    MFSR_REQUIRE(cfg != nullptr);
    TRY(validate(cfg));
    const int hrW = cfg->width * cfg->scale, hrH = cfg->height * cfg->scale;
    if (x0 == 0 && y0 == 0 && ((w == 0 && h == 0) || (w == hrW && h == hrH))) return MFSR_OK;  // the whole frame
    if (!mfsr_window_ok(hrW, hrH, x0, y0, w, h)) return MFSR_E_INVALID;
    if (!cfg->fused) return MFSR_E_UNSUPPORTED;  // (the unfused chain has no window kernels)
    return MFSR_OK;
}

extern "C" int mfsr_burst_set_window(mfsr_burst* b, int x0, int y0, int w, int h)
{
    MFSR_REQUIRE(b != nullptr);
    const int rc = mfsr_window_check(&b->cfg, x0, y0, w, h);
    if (rc != MFSR_OK) return rc;
    // between bursts only: a waiting frame would be fused into the other geometry
    if (b->pend.n > 0 || b->heldHas || b->nHold > 0) {
        fprintf(stderr, "mfsr: mfsr_burst_set_window with frames pending (flush or finish the burst first)\n");
        return MFSR_E_INVALID;
    }
    const Layout& L = b->L;
    const bool whole = (x0 == 0 && y0 == 0 && w == 0 && h == 0) || (x0 == 0 && y0 == 0 && w == L.hrW && h == L.hrH);
    b->winNext.on = !whole;
    b->winNext.x0 = whole ? 0 : x0;
    b->winNext.y0 = whole ? 0 : y0;
    b->winNext.w = whole ? 0 : w;
    b->winNext.h = whole ? 0 : h;
    return MFSR_OK;
}

extern "C" int mfsr_burst_get_window(const mfsr_burst* b, int* x0, int* y0, int* w, int* h)
{
    MFSR_REQUIRE(b && x0 && y0 && w && h);
    const mfsr_burst::Window& v = b->winNext;
    *x0 = v.on ? v.x0 : 0;
    *y0 = v.on ? v.y0 : 0;
    *w = v.on ? v.w : b->L.hrW;
    *h = v.on ? v.h : b->L.hrH;
    return MFSR_OK;
}

// B: coarse -> fine tile tracking of the moved pyramid against the reference's (refSq: the reference's sum(ref^2) per tile and
// level, fused tracker); the tile shifts of every level land in work.shifts
static int track_tiles(mfsr_burst* b, const FrameProducts& refF, float* const* refSq, const FrameProducts& movF,
                       const AlignScratch& work, const mfsr_prealign* hostBase, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const mfsr_float2 zero2 = {0.0f, 0.0f};
    for (int l = 0; l < c.levels; l++) {
        const int pi = ilog2(c.levelFactor[l]);
        const Img& ref = refF.pyr[pi];
        const Img& mov = movF.pyr[pi];
        const int T = c.tileSize[l], S = c.maxShift[l];
        const int tiles = L.tcx[l] * L.tcy[l];
        const mfsr_float2* pre = nullptr;
        b->paths[mfsr_trackTilesFastSupported(T, S) ? MFSR_PATH_TRACK_FAST_PAIR : MFSR_PATH_TRACK_GENERIC_PAIR]++;
        if (c.fused && l > 0) {
            // B8 folded into the tracker: the pre-shifts come straight from the previous level's shifts
            TRY(mfsr_trackTilesFusedUp((const float*)ref.ptr, (const float*)mov.ptr, (const mfsr_float2*)work.shifts[l - 1].ptr,
                                       work.shifts[l - 1].pitch, c.levelFactor[l - 1], c.levelFactor[l], L.tcx[l - 1], L.tcy[l - 1],
                                       c.tileSize[l - 1], (mfsr_float2*)work.shifts[l].ptr, work.shifts[l].pitch, ref.w, ref.h, ref.pitch, S,
                                       T, L.tcx[l], L.tcy[l], c.minimumThreshold, refSq[l], c.preAlign ? work.preResult : nullptr,
                                       1.0f / (float)c.levelFactor[l], stream));
            b->paths[MFSR_PATH_TRACK_FUSED_UP]++;
            continue;
        }
        if (l > 0) {
            TRY(mfsr_UpSampleShifts((const mfsr_float2*)work.shifts[l - 1].ptr, (mfsr_float2*)L.pre[l].ptr,
                                    work.shifts[l - 1].pitch, L.pre[l].pitch, c.levelFactor[l - 1], c.levelFactor[l],
                                    L.tcx[l - 1], L.tcy[l - 1], L.tcx[l], L.tcy[l], c.tileSize[l - 1], T, stream));
            pre = (const mfsr_float2*)L.pre[l].ptr;
        }
        if (c.fused) {
            TRY(mfsr_trackTilesFusedBase((const float*)ref.ptr, (const float*)mov.ptr, pre, L.pre[l].pitch,
                                         (mfsr_float2*)work.shifts[l].ptr, work.shifts[l].pitch, ref.w, ref.h, ref.pitch, S, T,
                                         L.tcx[l], L.tcy[l], c.minimumThreshold, refSq[l],
                                         c.preAlign ? work.preResult : nullptr, 1.0f / (float)c.levelFactor[l], stream));
            b->paths[MFSR_PATH_TRACK_FUSED_BASE]++;
        } else {
            b->paths[MFSR_PATH_TRACK_CHAIN]++;
            if (!pre) {
                MFSR_HIP_TRY(hipMemsetAsync(L.pre[l].ptr, 0, (size_t)L.pre[l].pitch * L.pre[l].h, mfsr_s(stream)));
                pre = (const mfsr_float2*)L.pre[l].ptr;
            }
            TRY(mfsr_convertToTilesOverlapBorder((const float*)ref.ptr, L.refTiles, ref.w, ref.h, ref.pitch, S, T, L.tcx[l],
                                                 L.tcy[l], zero2, 0.0f, stream));
            mfsr_float2 base = zero2;
            float rot = 0.0f;
            if (hostBase) {
                const float inv = 1.0f / (float)c.levelFactor[l];
                base.x = hostBase->shiftX * inv;
                base.y = hostBase->shiftY * inv;
                rot = hostBase->rotation;
            }
            TRY(mfsr_convertToTilesOverlapPreShift((const float*)mov.ptr, L.movTiles, pre, L.pre[l].pitch, mov.w, mov.h,
                                                   mov.pitch, S, T, L.tcx[l], L.tcy[l], base, rot, stream));
            TRY(mfsr_crossCorrelateTiles(L.refTiles, L.movTiles, L.cc, S, T, tiles, stream));
            TRY(mfsr_squaredSum(L.refTiles, L.sqsum, S, T, tiles, stream));
            TRY(mfsr_boxFilterWithBorderX(L.movTiles, L.boxX, S, T, tiles, stream));
            TRY(mfsr_boxFilterWithBorderY(L.boxX, L.boxY, S, T, tiles, stream));
            TRY(mfsr_normalizedCC(L.cc, L.sqsum, L.boxY, L.dist, S, T, tiles, stream));
            TRY(mfsr_findMinimum(L.dist, (mfsr_float2*)work.shifts[l].ptr, work.shifts[l].pitch, S, tiles, L.tcx[l],
                                 c.minimumThreshold, stream));
            TRY(mfsr_addRoundedPreShift(pre, L.pre[l].pitch, (mfsr_float2*)work.shifts[l].ptr, work.shifts[l].pitch, L.tcx[l],
                                        L.tcy[l], stream));
        }
    }
    return MFSR_OK;
}

// index of the upload slot (ring slot, or ring + i for reference slot i) that raw points to; -1 for caller-owned frames
static int upload_slot_of(const mfsr_burst* b, const uint16_t* raw)
{
    if (!raw) return -1;
    for (int i = 0; i < b->cfg.uploadRing; i++)
        if (b->L.rawRing[i] == raw) return i;
    for (int i = 0; i < 2; i++)
        if (b->cfg.uploadRing > 0 && b->L.refRaw[i] == raw) return b->cfg.uploadRing + i;
    return -1;
}

static int align_deferred(mfsr_burst* b, FuseGroup& g, mfsr_stream_t stream);

// ---- bookkeeping every fuse launch shares ---------------------------------------------------------------------------------
// Per-launch timing on request (mfsr_burst_timing): the event pair round a launch on `stream`.  *timed is handed on to timed_end,
// with the launches the pair stands for (1, or the groups of a burst launch) and the frames they fused.
static int timed_begin(mfsr_burst* b, mfsr_stream_t stream, bool* timed)
{
    *timed = b->timing && b->nEvents < kMaxTimedLaunches;
    if (*timed) {
        const int i = b->nEvents;
        if (!b->evStart[i]) MFSR_HIP_TRY(hipEventCreate(&b->evStart[i]));
        if (!b->evStop[i]) MFSR_HIP_TRY(hipEventCreate(&b->evStop[i]));
        MFSR_HIP_TRY(hipEventRecord(b->evStart[i], mfsr_s(stream)));
    }
    return MFSR_OK;
}
static int timed_end(mfsr_burst* b, bool timed, int launches, int frames, mfsr_stream_t stream)
{
    if (timed) {
        MFSR_HIP_TRY(hipEventRecord(b->evStop[b->nEvents], mfsr_s(stream)));
        b->evLaunches[b->nEvents] = launches;
        b->nEvents++;
        b->nFramesTimed += frames;
    }
    return MFSR_OK;
}

// mfsr_burst_begin(A, W): the first fuse onto A and W overwrites them (they are not zeroed or read)
static bool fresh_for(const mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights)
{
    return b->fresh.has && b->fresh.imgOut == imgOut && b->fresh.totalWeights == totalWeights;
}
// ... and the zeroes A and W are owed when nothing overwrites them
static int zero_fresh(mfsr_burst* b, mfsr_stream_t stream)
{
    const size_t bytes = acc_bytes(b);
    MFSR_HIP_TRY(hipMemsetAsync(b->fresh.imgOut, 0, bytes, mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemsetAsync(b->fresh.totalWeights, 0, bytes, mfsr_s(stream)));
    b->fresh.has = false;
    return MFSR_OK;
}
// The fresh decision of a fuse onto imgOut / totalWeights on `stream`: *freshNow = this fuse is the overwriting one.  A fuse into
// other accumulators than those of mfsr_burst_begin: A and W get their zeroes here.  Either way the burst is fresh no longer.
static int take_fresh(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, mfsr_stream_t stream, int* freshNow)
{
    *freshNow = fresh_for(b, imgOut, totalWeights);
    if (b->fresh.has && !*freshNow) TRY(zero_fresh(b, stream));
    b->fresh.has = false;
    return MFSR_OK;
}

// upload slots whose raw frame the group's launch on `stream` was the last to read may be overwritten once it has run
static int release_group_slots(mfsr_burst* b, const FuseGroup& g, mfsr_stream_t stream)
{
    if (!b->copyStream) return MFSR_OK;
    for (int j = 0; j < g.n; j++) {
        const int us = upload_slot_of(b, g.raw[j]);
        if (us >= 0) TRY(record_free(b, us, stream));
    }
    return MFSR_OK;
}

// a ring slot's buffers are free once the fuse that read them last has run: `stream` is about to rewrite them
static int wait_slot_fused(mfsr_burst* b, int slot, mfsr_stream_t stream)
{
    if (b->fuseStream && b->fusedOutstanding[slot]) {
        MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evFused[slot], 0));
        b->fusedOutstanding[slot] = false;
    }
    return MFSR_OK;
}

// between bursts: no group waits anywhere and no packed upload waits for its unpack
static bool burst_idle(const mfsr_burst* b) { return b->pend.n == 0 && !b->heldHas && b->nHold == 0 && b->nUnp == 0; }

// ---- burst hold -------------------------------------------------------------------------------------------------------------
// Process-wide switch of the burst hold for A/B (mfsr_set_burst_fuse; MFSR_BURST_FUSE=0 in the environment): off, every
// context fuses its groups as they complete, whatever mfsr_burst_hold_fuse said.
static MfsrKnob g_burst_fuse;
static bool burst_fuse_enabled()
{
    return g_burst_fuse.get([] { return mfsr_env_is0("MFSR_BURST_FUSE") ? 0 : 1; }) == 1;
}
extern "C" int mfsr_set_burst_fuse(int enable)
{
    g_burst_fuse.set(enable ? 1 : 0);
    return MFSR_OK;
}
// Process-wide switch of the finish inside the burst launch for A/B (mfsr_set_finish_fuse; MFSR_FINISH_FUSE=0 in the
// environment): off, mfsr_burst_finish always runs its finish pass.
static MfsrKnob g_finish_fuse;
static bool finish_fuse_enabled()
{
    return g_finish_fuse.get([] { return mfsr_env_is0("MFSR_FINISH_FUSE") ? 0 : 1; }) == 1;
}
extern "C" int mfsr_set_finish_fuse(int enable)
{
    g_finish_fuse.set(enable ? 1 : 0);
    return MFSR_OK;
}
extern "C" int mfsr_burst_debug_finish_fused(const mfsr_burst* b, int* finishes)
{
    MFSR_REQUIRE(b && finishes);
    *finishes = b->fusedFinishes;
    return MFSR_OK;
}
extern "C" int mfsr_burst_hold_fuse(mfsr_burst* b, int enable)
{
    MFSR_REQUIRE(b != nullptr);
    b->holdFuse = enable != 0;  // (groups already held leave with the next flush / finish / add_frame that needs their slots)
    return MFSR_OK;
}
extern "C" int mfsr_burst_fuse_stats(const mfsr_burst* b, int* burstLaunches, int* groupsFused)
{
    MFSR_REQUIRE(b && burstLaunches && groupsFused);
    *burstLaunches = b->burstLaunches;
    *groupsFused = b->burstGroups;
    return MFSR_OK;
}

// may the complete, aligned group in b->pend wait for the burst launch?  Only the plain resident path of the x2 Bayer tile
// geometry: everything else (asyncFuse, windows, host bursts, frames in upload slots, other group sizes) fuses as before.
static bool can_hold_group(const mfsr_burst* b, bool hostBurst)
{
    const mfsr_config& c = b->cfg;
    if (!b->holdFuse || !burst_fuse_enabled() || hostBurst || b->heldHas || b->fuseStream || b->win.on) return false;
    if (!c.fused || c.mono || c.scale != 2 || b->group != MFSR_MAX_FUSE_GROUP || b->pend.n != MFSR_MAX_FUSE_GROUP) return false;
    if (b->L.tw * 2 != b->L.W || b->L.th * 2 != b->L.H) return false;
    if (b->nHold >= MFSR_MAX_BURST_FUSE / MFSR_MAX_FUSE_GROUP) return false;
    if (b->nHold > 0 && (b->hold[0].imgOut != b->pend.imgOut || b->hold[0].totalWeights != b->pend.totalWeights)) return false;
    for (int i = 0; i < b->pend.n; i++)
        if (upload_slot_of(b, b->pend.raw[i]) >= 0) return false;
    return true;
}

// G: one aligned group (1 .. MFSR_MAX_FUSE_GROUP frames) onto its accumulators as the ordinary launch, with all of its
// bookkeeping (timed with HIP events on request)
static int launch_group(mfsr_burst* b, const FuseGroup& g, mfsr_stream_t callerStream)
{
    const int n = g.n;
    if (n == 0) return MFSR_OK;
    // with asyncFuse the launch goes to the burst's own stream, ordered after the alignment of its frames
    mfsr_stream_t stream = callerStream;
    if (b->fuseStream) {
        stream = (mfsr_stream_t)b->fuseStream;
        for (int i = 0; i < n; i++) MFSR_HIP_TRY(hipStreamWaitEvent(b->fuseStream, b->evAligned[g.slot[i]], 0));
    }
    bool timed;
    TRY(timed_begin(b, stream, &timed));
    int freshNow;
    TRY(take_fresh(b, g.imgOut, g.totalWeights, stream, &freshNow));
    TRY(fuse_group(b, g, freshNow, 0, out_h(b), stream));
    TRY(timed_end(b, timed, 1, n, stream));
    TRY(release_group_slots(b, g, stream));
    if (b->fuseStream) {
        for (int i = 0; i < n; i++) {
            MFSR_HIP_TRY(hipEventRecord(b->evFused[g.slot[i]], b->fuseStream));
            b->fusedOutstanding[g.slot[i]] = true;
        }
    }
    return MFSR_OK;
}

// The groups that wait outside the filling group onto their accumulators, in arrival order: the burst hold's first (a held
// group can only have arrived after every one of them: can_hold_group refuses while one is held), then -- heldToo -- the host
// burst's held group.  Two or more hold groups leave as ONE launch (counted as one timed launch per group, so that
// mfsr_burst_timing_read's average stays "per four-frame group"); a single one, or a geometry the burst kernel does not take,
// as the ordinary launches they would have been, and so does the held group: exactly as if it had not been held.
// (heldToo = false: callers that only need the hold's ring slots, and mfsr_burst_finish_host, which fuses `held` band by band)
static int drain_waiting(mfsr_burst* b, mfsr_stream_t stream, bool heldToo = true)
{
    const int G = b->nHold;
    b->nHold = 0;
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    int rc = MFSR_E_UNSUPPORTED;
    if (G >= 2) {
        const uint16_t* raws[MFSR_MAX_BURST_FUSE];
        mfsr_tex2d masks[MFSR_MAX_BURST_FUSE], flows[MFSR_MAX_BURST_FUSE];
        for (int g = 0; g < G; g++) {
            const int k = g * MFSR_MAX_FUSE_GROUP;
            for (int i = 0; i < MFSR_MAX_FUSE_GROUP; i++) raws[k + i] = b->hold[g].raw[i];
            group_tables(b->hold[g], masks + k, flows + k);
        }
        mfsr_float3* imgOut = b->hold[0].imgOut;
        mfsr_float3* totalWeights = b->hold[0].totalWeights;
        mfsr_tex2d acc[2];
        for (int p = 0; p < 2; p++) {
            acc[p].ptr = p ? (void*)totalWeights : (void*)imgOut;
            acc[p].pitch = 12 * L.hrW;
            acc[p].width = L.hrW;
            acc[p].height = L.hrH;
        }
        int freshNow = fresh_for(b, imgOut, totalWeights);  // (taken after the launch: an entry that refuses leaves the burst fresh)
        bool timed;
        TRY(timed_begin(b, stream, &timed));
        const mfsr_float3 white = cfg_white(c), black = cfg_black(c);
        // the burst's last fuse and a plain uint16_t finish waiting behind it (mfsr_burst_finish): the launch finishes as well
        uint16_t* const out16 = b->finishOut16;
        b->finishOut16 = nullptr;
        if (out16) {
            mfsr_tex2d fb;  // as mfsr_burst_finish hands it to mfsr_finishFused: the LR image at its pitch
            fb.ptr = L.fallback.ptr;
            fb.pitch = L.fallback.pitch;
            fb.width = L.W;
            fb.height = L.H;
            rc = mfsr_cfa::accumulateSuperResBurstFinish(b->cfa, G * MFSR_MAX_FUSE_GROUP, raws, acc[0], acc[1], masks, as_tex(L.kparam4), flows, white,
                                                    black, c.scale, freshNow, fb, 0.0f, 1.0f, 0.0f, 1.0f, c.weightThreshold, out16,
                                                    L.hrW, L.hrH, 0, 65535.0f, 0, 0, L.hrW, L.hrH, stream);
            if (rc == MFSR_OK) {
                b->finishTaken = true;
                b->fusedFinishes++;
            }
        }
        if (rc == MFSR_E_UNSUPPORTED)
            rc = mfsr_cfa::accumulateSuperResBurst(b->cfa, G * MFSR_MAX_FUSE_GROUP, raws, acc[0], acc[1], masks, as_tex(L.kparam4), flows, white, black,
                                              c.scale, freshNow, stream);
        if (rc == MFSR_OK) {
            TRY(take_fresh(b, imgOut, totalWeights, stream, &freshNow));
            b->burstLaunches++;
            b->burstGroups += G;
            TRY(timed_end(b, timed, G, G * MFSR_MAX_FUSE_GROUP, stream));
        } else if (rc != MFSR_E_UNSUPPORTED)
            return rc;
    }
    // (a refusal touched nothing)
    for (int g = 0; g < G && rc == MFSR_E_UNSUPPORTED; g++) {
        TRY(wait_uploads(b, stream));
        TRY(launch_group(b, b->hold[g], stream));
    }
    if (!heldToo || !b->heldHas) return MFSR_OK;
    const FuseGroup held = b->held;
    b->heldHas = false;
    b->held.n = 0;
    TRY(wait_uploads(b, stream));
    return launch_group(b, held, stream);
}

// the filling group onto its accumulators, behind everything that arrived before it
static int accumulate_pending(mfsr_burst* b, mfsr_stream_t stream)
{
    TRY(drain_waiting(b, stream));
    TRY(align_deferred(b, b->pend, stream));  // frames of the group that were waiting for their batch
    TRY(wait_uploads(b, stream));             // (a reference frame of the group is read by the fuse only)
    const FuseGroup g = b->pend;
    b->pend.n = 0;
    return launch_group(b, g, stream);
}

// `stream` is about to read the kernel parameters / the fallback image: wait for the launches that make them
static int wait_ref_products(mfsr_burst* b, mfsr_stream_t stream)
{
    if (b->refOnFuse && mfsr_s(stream) != b->fuseStream) MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evRefDone, 0));
    return MFSR_OK;
}

// the caller's stream waits for every fuse issued so far, and for the reference products (no-op without asyncFuse)
static int join_fuse(mfsr_burst* b, mfsr_stream_t stream)
{
    if (!b->fuseStream) return MFSR_OK;
    TRY(wait_ref_products(b, stream));
    for (int i = 0; i < b->ring; i++)
        if (b->fusedOutstanding[i]) {
            MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evFused[i], 0));
            b->fusedOutstanding[i] = false;
        }
    return MFSR_OK;
}

// fuse the frames still waiting for the rest of their group, then join: afterwards the caller's stream sees every frame
static int flush_pending(mfsr_burst* b, mfsr_stream_t stream, bool materializeFresh)
{
    // mfsr_burst_begin with no frame fused since: the accumulators must read as zero
    if (materializeFresh && b->fresh.has && b->pend.n == 0 && !b->heldHas && b->nHold == 0) TRY(zero_fresh(b, stream));
    TRY(accumulate_pending(b, stream));
    return join_fuse(b, stream);
}

static bool lk_warped_path(const mfsr_burst* b)
{
    // fused LK: the warped moved image travels from launch to launch (every pixel warped once per iteration, by the
    // thread that has just updated its flow) instead of being re-gathered for every tile halo; MFSR_LK_WARPED=0: A/B
    static const bool lkWarped = !mfsr_env_is0("MFSR_LK_WARPED");
    const mfsr_config& c = b->cfg;
    return c.fused && lkWarped && c.lkIterations > 0 && b->L.tw >= 64 && b->L.th >= 32;
}

// Which buffer of the slot's LK ping-pong pair holds a frame's final flow.  Every fused iteration (sweep, warped or plain) writes
// the pair's other buffer, so an odd number of them ends in buffer 1; the unfused chain updates buffer 0 in place; without
// iterations the flow field stays where it was made, in buffer 0 -- as does a reference frame's identity flow.
static const Img* final_flow(const mfsr_burst* b, int slot, int isReference)
{
    const mfsr_config& c = b->cfg;
    return &b->L.flowBuf[2 * slot + (!isReference && c.fused ? (c.lkIterations & 1) : 0)];
}

// One frame's alignment into ring slot `slot` is three stages.  mov / work: the frame's products and the scratch its alignment
// writes; prepared: mov was made by the caller (frame streams, joint mode); suppliedShifts: tile shifts that replace the
// tracker's (joint mode).
// align_pre: A1 + tracking pyramid, (I) pre-alignment, B tracker, D1 flow field (+ first warp) -- everything up to the
// Lucas-Kanade iterations; for the reference frame the identity flow and certainty 1, which is all of its alignment.
static int align_pre(mfsr_burst* b, const uint16_t* raw, int isReference, int slot, const FrameProducts& mov, bool prepared,
                     const AlignScratch& work, const Img* suppliedShifts, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const FrameProducts& ref = b->ref;
    TRY(wait_uploads(b, stream));
    TRY(wait_slot_fused(b, slot, stream));
    const Img* flow = &L.flowBuf[2 * slot];
    if (isReference) {
        const Img* mask = &L.maskBuf[slot];
        MFSR_HIP_TRY(hipMemsetAsync(flow->ptr, 0, (size_t)flow->pitch * flow->h, mfsr_s(stream)));
        return mfsr_fill_f32((float*)mask->ptr, (size_t)mask->pitch / 4 * mask->h, 1.0f, stream);
    }
    if (!prepared) TRY(prepare_frame(b, raw, mov, stream));
    // I: global pre-alignment (base shift + rotation of this frame against the reference), kept in device memory
    mfsr_prealign hostBase;
    const mfsr_prealign* hb = nullptr;
    if (c.preAlign) {
        if (!prepared) TRY(mfsr_preAlignPyramid((const float*)mov.pyr[0].ptr, L.tw, L.th, mov.pyr[0].pitch, mov.prePyr, stream));
        TRY(mfsr_preAlign(ref.prePyr, mov.prePyr, L.tw, L.th, c.preAlignMaxAngle, L.preWork, work.preResult, stream));
        b->preCur = work.preResult;
        if (!c.fused) {
            // the reference-shaped entry points take baseShift / baseRotation by value: one host round trip
            MFSR_HIP_TRY(hipMemcpyAsync(&hostBase, work.preResult, sizeof(hostBase), hipMemcpyDeviceToHost, mfsr_s(stream)));
            MFSR_HIP_TRY(hipStreamSynchronize(mfsr_s(stream)));
            hb = &hostBase;
        }
    }
    if (!suppliedShifts) TRY(track_tiles(b, ref, L.refSq, mov, work, hb, stream));
    const int last = c.levels - 1;
    const Img& tileShifts = suppliedShifts ? *suppliedShifts : work.shifts[last];
    const mfsr_float2 zero2 = {0.0f, 0.0f};
    if (lk_warped_path(b)) {
        TRY(mfsr_CreateFlowFieldWarped((mfsr_float2*)flow->ptr, as_tex(tileShifts), L.tw, L.th, flow->pitch, zero2, 0.0f,
                                       c.preAlign ? work.preResult : nullptr, (const float*)ref.pyr[0].ptr,
                                       (const float*)mov.pyr[0].ptr, ref.pyr[0].pitch, (float*)work.lkSum[0].ptr,
                                       (float*)work.lkDiff[0].ptr, work.lkSum[0].pitch, stream));
        b->paths[MFSR_PATH_FLOW_WARPED]++;
    } else if (c.preAlign && c.fused) {
        TRY(mfsr_CreateFlowFieldFromTilesBase((mfsr_float2*)flow->ptr, as_tex(tileShifts), L.tw, L.th, flow->pitch, work.preResult,
                                              stream));
        b->paths[MFSR_PATH_FLOW_BASE]++;
    } else {
        mfsr_float2 base = zero2;
        float rot = 0.0f;
        if (hb) {
            base.x = hb->shiftX;
            base.y = hb->shiftY;
            rot = hb->rotation;
        }
        TRY(mfsr_CreateFlowFieldFromTiles((mfsr_float2*)flow->ptr, as_tex(tileShifts), c.tileSize[last], L.tcx[last], L.tcy[last],
                                          L.tw, L.th, flow->pitch, base, rot, stream));
        b->paths[MFSR_PATH_FLOW_PLAIN]++;
    }
    return MFSR_OK;
}

// one frame of a sweep launch, iteration `it` of the fused Lucas-Kanade: the slot's flow pair and the frame's running sums ping-pong
static mfsr_lk_frame lk_frame_desc(const Layout& L, int slot, int it, bool lastIt, const FrameProducts& mov, const AlignScratch& work)
{
    const int in = it & 1, out = in ^ 1;
    mfsr_lk_frame f;
    f.shiftsIn = (const mfsr_float2*)L.flowBuf[2 * slot + in].ptr;
    f.shiftsOut = (mfsr_float2*)L.flowBuf[2 * slot + out].ptr;
    f.movedImg = (const float*)mov.pyr[0].ptr;
    f.sumIn = (const float*)work.lkSum[in].ptr;
    f.diffIn = (const float*)work.lkDiff[in].ptr;
    f.sumOut = lastIt ? nullptr : (float*)work.lkSum[out].ptr;
    f.diffOut = lastIt ? nullptr : (float*)work.lkDiff[out].ptr;
    return f;
}

// the fused prepare launch's table for the moved frames of a batch: the frame at batch position mq[k] is g's frame idx[mq[k]]
static void prepare_table(const Layout& L, const FuseGroup& g, const int* idx, const int* mq, int m, mfsr_prepare_frame* pf)
{
    const int nlev = ilog2(L.maxFactor) + 1;
    for (int k = 0; k < m; k++) {
        const Img* pyr = L.mov[mq[k]].pyr;
        pf[k].dataIn = g.raw[idx[mq[k]]];
        pf[k].halfOut = (mfsr_float3*)L.mov[mq[k]].half.ptr;
        pf[k].pyr0 = (float*)pyr[0].ptr;
        pf[k].pyr1 = nlev > 1 ? (float*)pyr[1].ptr : nullptr;
    }
}

// align_lk: K, the Lucas-Kanade iterations of one moved frame, launch by launch; the flow ends in final_flow(b, slot, 0)
static int align_lk(mfsr_burst* b, int slot, const FrameProducts& mov, const AlignScratch& work, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const FrameProducts& ref = b->ref;
    const bool warped = lk_warped_path(b);
    for (int it = 0; it < c.lkIterations; it++) {
        const bool lastIt = it == c.lkIterations - 1;
        const int in = it & 1, out = in ^ 1;
        const float scale = lastIt ? (float)L.flowScale : 1.0f;  // the fused LK scales on its last iteration
        const Img* flow = &L.flowBuf[2 * slot + (c.fused ? in : 0)];
        const Img* other = &L.flowBuf[2 * slot + out];
        if (warped) {
            // the sweep kernel wherever it applies, also for a single frame: the frame-by-frame paths (frame streams,
            // joint mode, mfsr_burst_align_frame of the multi-GPU layer, groups of one) then give the very bits of the
            // frame-batched burst -- its result does not depend on how many frames share a launch
            const mfsr_lk_frame one = lk_frame_desc(L, slot, it, lastIt, mov, work);
            const int rcs = mfsr_lucasKanadeSweepBatch(1, &one, (const float*)ref.pyr[0].ptr, flow->pitch, ref.pyr[0].pitch,
                                                       work.lkSum[0].pitch, L.tw, L.th, c.lkHalfWindow, c.lkMinDet, scale, stream);
            if (rcs != MFSR_E_UNSUPPORTED) {
                if (rcs) return rcs;
                b->paths[MFSR_PATH_LK_SWEEP_SINGLE]++;
                continue;
            }
            TRY(mfsr_lucasKanadeIterationWarped((const mfsr_float2*)flow->ptr, (mfsr_float2*)other->ptr, flow->pitch,
                                                (const float*)ref.pyr[0].ptr, (const float*)mov.pyr[0].ptr, ref.pyr[0].pitch,
                                                one.sumIn, one.diffIn, one.sumOut, one.diffOut, work.lkSum[0].pitch, L.tw, L.th,
                                                c.lkHalfWindow, c.lkMinDet, scale, stream));
            b->paths[MFSR_PATH_LK_ITERATION_WARPED]++;
        } else if (c.fused) {
            TRY(mfsr_lucasKanadeIterationFused((const mfsr_float2*)flow->ptr, (mfsr_float2*)other->ptr, flow->pitch,
                                               (const float*)ref.pyr[0].ptr, (const float*)mov.pyr[0].ptr, ref.pyr[0].pitch, L.tw, L.th,
                                               c.lkHalfWindow, c.lkMinDet, scale, stream));
            b->paths[MFSR_PATH_LK_ITERATION_FUSED]++;
        } else {
            TRY(mfsr_WarpingKernel(L.tw, L.th, L.warped.pitch, as_tex(*flow), (float*)L.warped.ptr, as_tex(mov.pyr[0]), stream));
            // texSource = warped moved frame, texTarget = reference: the reference's stencil is
            // minus the usual derivative (opticalFlow.cu:116-119) and Iz = source - target (:131),
            // so this is the order for which `shift += UV` (:322-323) descends.
            TRY(mfsr_ComputeDerivativesKernel(L.tw, L.th, L.Ix.pitch, (float*)L.Ix.ptr, (float*)L.Iy.ptr, (float*)L.It.ptr,
                                              as_tex(L.warped), as_tex(ref.pyr[0]), stream));
            TRY(mfsr_lucasKanadeOptim((mfsr_float2*)flow->ptr, (const float*)L.Ix.ptr, (const float*)L.Iy.ptr, (const float*)L.It.ptr,
                                      flow->pitch, L.Ix.pitch, L.tw, L.th, c.lkHalfWindow, c.lkMinDet, stream));
            b->paths[MFSR_PATH_LK_CHAIN]++;
        }
    }
    if (L.flowScale != 1 && !(c.fused && c.lkIterations > 0)) {
        const Img* flow = final_flow(b, slot, 0);
        TRY(mfsr_scaleFlow((mfsr_float2*)flow->ptr, flow->pitch, L.tw, L.th, (float)L.flowScale, stream));
        b->paths[MFSR_PATH_SCALE_FLOW]++;
    }
    return MFSR_OK;
}

// align_post: F, the robustness mask of one moved frame from its final flow (the 1-px ring is never written by the kernel ->
// zero it); with cfg.maskErode into the scratch mask, from which the erosion writes the slot's
static int align_post(mfsr_burst* b, int slot, const FrameProducts& mov, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const FrameProducts& ref = b->ref;
    const Img* flow = final_flow(b, slot, 0);
    const Img* mask = &L.maskBuf[slot];
    const Img* fOut = c.maskErode > 0 ? &L.maskRaw[0] : mask;
    if (c.fused) {
        TRY(mfsr_robustnessMaskFused((const mfsr_float3*)ref.half.ptr, (const mfsr_float3*)mov.half.ptr, (mfsr_float4*)fOut->ptr,
                                     as_tex(*flow), L.hw, L.hh, ref.half.pitch, fOut->pitch, c.alpha, c.beta, c.thresholdM, stream));
        b->paths[MFSR_PATH_ROBUST_FUSED]++;
    } else {
        b->paths[MFSR_PATH_ROBUST_CHAIN]++;
        TRY(mfsr_zeroRing_f32x4((mfsr_float4*)fOut->ptr, fOut->pitch, L.hw, L.hh, stream));
        TRY(mfsr_ComputeRobustnessMask((const mfsr_float3*)ref.half.ptr, (const mfsr_float3*)mov.half.ptr, (mfsr_float4*)fOut->ptr,
                                       as_tex(*flow), L.hw, L.hh, ref.half.pitch, fOut->pitch, c.alpha, c.beta, c.thresholdM, stream));
    }
    if (c.maskErode > 0) {
        const mfsr_float4* ein = (const mfsr_float4*)fOut->ptr;
        mfsr_float4* eout = (mfsr_float4*)mask->ptr;
        TRY(mfsr_erodeMaskBatch(1, &ein, &eout, L.hw, L.hh, fOut->pitch, mask->pitch, c.maskErode, stream));
    }
    return MFSR_OK;
}

// the flow and the mask of an aligned frame: where mfsr_burst_debug_frame_views and the fuse find them
static void aligned_outputs(mfsr_burst* b, int slot, int isReference, const Img** flowOut, const Img** maskOut)
{
    *flowOut = b->slotFlow[slot] = final_flow(b, slot, isReference);
    *maskOut = &b->L.maskBuf[slot];
}

// A1 + (I) + B + D + F of one frame into ring slot `slot`, in the burst's first set of per-frame intermediates (or from the
// products / with the tile shifts the caller supplies): *flowOut / *maskOut name the buffers that hold the result
static int align_frame(mfsr_burst* b, const uint16_t* raw, int isReference, int slot, const FrameProducts* prepared,
                       const Img* suppliedShifts, const Img** flowOut, const Img** maskOut, mfsr_stream_t stream)
{
    const FrameProducts& mov = prepared ? *prepared : b->L.mov[0];
    const AlignScratch& work = b->L.work[0];
    TRY(align_pre(b, raw, isReference, slot, mov, prepared != nullptr, work, suppliedShifts, stream));
    if (!isReference) {
        TRY(align_lk(b, slot, mov, work, stream));
        TRY(align_post(b, slot, mov, stream));
    }
    aligned_outputs(b, slot, isReference, flowOut, maskOut);
    return MFSR_OK;
}

// MFSR_ALIGN_BATCH (A/B): 0 = every frame is aligned on its own; 1s = a group shares its Lucas-Kanade launches only; anything
// else, or unset = a group shares every stage the batch kernels serve
enum AlignBatch { ALIGN_BATCH_OFF, ALIGN_BATCH_LK, ALIGN_BATCH_STAGES };
static AlignBatch align_batch_mode()
{
    static const AlignBatch mode = [] {
        const char* e = getenv("MFSR_ALIGN_BATCH");
        if (e && e[0] == '0') return ALIGN_BATCH_OFF;
        return e && e[0] == '1' && e[1] == 's' ? ALIGN_BATCH_LK : ALIGN_BATCH_STAGES;
    }();
    return mode;
}

// Frame-batched alignment.  The frames of a fuse group are independent given the reference's products, and one frame's
// alignment is a chain of small launches (prepare, two tracker levels, flow field, lkIterations x Lucas-Kanade, robustness:
// 8 at the defaults, 10..30 us each at 4K) -- so add_frame only REGISTERS a frame while its group fills, and the group is
// aligned as one batch when it is complete (or on flush / finish): the per-frame stages frame after frame into per-frame
// intermediates (Layout::mov / Layout::work), every Lucas-Kanade iteration of all frames in ONE launch (mfsr_lucasKanadeSweepBatch).
// Same kernels' arithmetic per frame as the frame-by-frame path except the sweep kernel's row-sum order (fp32 rounding of
// the flow).  Frames whose products or tile shifts the caller supplies (frame streams, the joint mode: `supplied`) take the
// frame-by-frame path.
static bool can_defer_alignment(const mfsr_burst* b, bool supplied)
{
    const mfsr_config& c = b->cfg;
    // (host bursts: frames are aligned one by one as they come off the PCIe link -- waiting for a whole group would leave
    // the GPU idle during the first uploads and would put the whole last group's alignment between the last upload and
    // the first byte of the download; MFSR_HOST_DEFER=1 batches the groups after the first anyway)
    static const bool hostDefer = mfsr_env_is1("MFSR_HOST_DEFER");
    // ... and a host burst that was enqueued while the previous one was still being fused and downloaded (bursts back to
    // back: b->hostBusy) batches every group: the GPU has work queued, so frame-by-frame launches buy no latency and cost
    // a tenth of the alignment's throughput
    const bool hostImmediate = b->holdLastGroup && !b->hostBusy && (b->framesSinceRef < b->group || !hostDefer);
    // (the sweep's own rule for the layout's images: what it admits here it takes in align_deferred)
    const Layout& L = b->L;
    return align_batch_mode() != ALIGN_BATCH_OFF && b->group > 1 && L.nAlign >= b->group && lk_warped_path(b) && !supplied &&
           !hostImmediate &&
           mfsr_lk_sweep_accepts(b->group, L.tw, L.th, c.lkHalfWindow, L.flowBuf[0].pitch, b->ref.pyr[0].pitch, L.work[0].lkSum[0].pitch) ==
               MFSR_OK;
}

static int align_deferred(mfsr_burst* b, FuseGroup& g, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const FrameProducts& ref = b->ref;
    int idx[MFSR_MAX_FUSE_GROUP], n = 0;
    for (int i = 0; i < g.n; i++)
        if (g.deferred[i]) idx[n++] = i;
    if (n == 0) return MFSR_OK;
    TRY(wait_uploads(b, stream));
    b->paths[MFSR_PATH_ALIGN_BATCHES]++;
    // The frame at batch position q works in L.mov[q] / L.work[q].
    // Every per-frame stage as ONE launch over the batch (gridDim.z = frame) where the default kernels apply: the fused prepare
    // kernel, the compile-time tracker at every level, the flow field + first warp, later the fused robustness kernel.
    // Anything else (monochrome frames, pre-alignment, other tile sizes) runs the same stages frame by frame.
    const int nlev = ilog2(L.maxFactor) + 1;
    bool stageBatch = align_batch_mode() == ALIGN_BATCH_STAGES && c.fused && !c.mono && !c.preAlign && b->ntaps / 2 <= 8 &&
                      L.tw == L.hw && L.th == L.hh;
    for (int l = 0; l < c.levels && stageBatch; l++) stageBatch = mfsr_trackTilesFastSupported(c.tileSize[l], c.maxShift[l]) != 0;
    int mq[MFSR_MAX_FUSE_GROUP], m = 0;  // batch positions of the moved (non-reference) frames
    for (int q = 0; q < n; q++)
        if (!g.isRef[idx[q]]) mq[m++] = q;
    // The masks of the group in one pass (mfsr_robustnessMaskGroup): the prepare launch then leaves the 3 x 3 patch MEANS of the
    // half-resolution image in L.mov[q].half, which on this path only the mask kernel reads.  Decided once, here, for both launches.
    const bool maskGroup = stageBatch && m > 0 && b->ntaps >= 3 && mfsr_robustness_group() != 0 &&
                           mfsr_robustness_group_fits(L.hh, L.flowBuf[0].pitch, L.mov[0].half.pitch, L.maskBuf[0].pitch) != 0;
    if (stageBatch) {
        b->paths[MFSR_PATH_STAGE_BATCHES]++;
        for (int q = 0; q < n; q++) {
            const int i = idx[q], slot = g.slot[i];
            if (g.isRef[i]) {  // identity flow, certainty 1 (and the slot wait) through the frame path
                TRY(align_pre(b, g.raw[i], 1, slot, L.mov[q], false, L.work[q], nullptr, stream));
            } else
                TRY(wait_slot_fused(b, slot, stream));
        }
        if (m > 0) {
            // A1 + luma + prefilter + first pyramid level
            mfsr_prepare_frame pf[MFSR_MAX_FUSE_GROUP];
            prepare_table(L, g, idx, mq, m, pf);
            TRY(mfsr_cfa::prepareFrames(b->cfa, m, pf, L.mov[0].half.pitch, c.maxVal, L.hw, L.hh, L.mov[0].pyr[0].pitch,
                                        nlev > 1 ? L.mov[0].pyr[1].pitch : 0, b->taps, b->ntaps, stream, maskGroup));
            b->paths[MFSR_PATH_PREPARE_BATCH]++;
            for (int k = 0; k < m; k++) {
                const Img* pyr = L.mov[mq[k]].pyr;
                for (int i = 2; i < nlev; i++)
                    TRY(mfsr_downsample2x((const float*)pyr[i - 1].ptr, pyr[i - 1].pitch, (float*)pyr[i].ptr, pyr[i].pitch, pyr[i].w, pyr[i].h,
                                          stream));
            }
            // B: coarse -> fine, one launch per level
            for (int l = 0; l < c.levels; l++) {
                const int pi = ilog2(c.levelFactor[l]);
                mfsr_track_frame tf[MFSR_MAX_FUSE_GROUP];
                for (int k = 0; k < m; k++) {
                    tf[k].movedImg = (const float*)L.mov[mq[k]].pyr[pi].ptr;
                    tf[k].coarseShifts = l > 0 ? (const mfsr_float2*)L.work[mq[k]].shifts[l - 1].ptr : nullptr;
                    tf[k].coordinates = (mfsr_float2*)L.work[mq[k]].shifts[l].ptr;
                    tf[k].base = nullptr;
                }
                const Img& refImg = ref.pyr[pi];
                const Img* shifts = L.work[0].shifts;  // (every frame's tile grids have these pitches)
                TRY(mfsr_trackTilesFusedBatch(m, tf, (const float*)refImg.ptr, l > 0 ? shifts[l - 1].pitch : 0, l > 0 ? c.levelFactor[l - 1] : 0,
                                              c.levelFactor[l], l > 0 ? L.tcx[l - 1] : 0, l > 0 ? L.tcy[l - 1] : 0,
                                              l > 0 ? c.tileSize[l - 1] : 0, shifts[l].pitch, refImg.w, refImg.h, refImg.pitch, c.maxShift[l],
                                              c.tileSize[l], L.tcx[l], L.tcy[l], c.minimumThreshold, L.refSq[l],
                                              1.0f / (float)c.levelFactor[l], stream));
                b->paths[MFSR_PATH_TRACK_FUSED_BATCH]++;
                b->paths[MFSR_PATH_TRACK_FAST_PAIR]++;  // (stageBatch: every level's pair is one of the compile-time tracker's)
            }
            // D1 + the first warp
            const int last = c.levels - 1;
            mfsr_flowfield_frame ff[MFSR_MAX_FUSE_GROUP];
            for (int k = 0; k < m; k++) {
                const int slot = g.slot[idx[mq[k]]];
                ff[k].outImg = (mfsr_float2*)L.flowBuf[2 * slot].ptr;
                ff[k].tileShifts = (const mfsr_float2*)L.work[mq[k]].shifts[last].ptr;
                ff[k].base = nullptr;
                ff[k].movedImg = (const float*)L.mov[mq[k]].pyr[0].ptr;
                ff[k].sumOut = (float*)L.work[mq[k]].lkSum[0].ptr;
                ff[k].diffOut = (float*)L.work[mq[k]].lkDiff[0].ptr;
            }
            const Img& grid = L.work[0].shifts[last];
            TRY(mfsr_CreateFlowFieldWarpedBatch(m, ff, grid.pitch, grid.w, grid.h, L.tw, L.th, L.flowBuf[0].pitch,
                                                (const float*)ref.pyr[0].ptr, ref.pyr[0].pitch, L.work[0].lkSum[0].pitch, stream));
            b->paths[MFSR_PATH_FLOW_WARPED_BATCH]++;
        }
    } else {
        // per-frame stages up to the flow field + first warp
        for (int q = 0; q < n; q++) {
            const int i = idx[q];
            TRY(align_pre(b, g.raw[i], g.isRef[i], g.slot[i], L.mov[q], false, L.work[q], nullptr, stream));
        }
    }
    // every Lucas-Kanade iteration of the batch in one launch
    for (int it = 0; it < c.lkIterations; it++) {
        mfsr_lk_frame fr[MFSR_MAX_FUSE_GROUP];
        int m = 0;
        const bool lastIt = it == c.lkIterations - 1;
        for (int q = 0; q < n; q++)
            if (!g.isRef[idx[q]]) fr[m++] = lk_frame_desc(L, g.slot[idx[q]], it, lastIt, L.mov[q], L.work[q]);
        if (m == 0) break;
        TRY(mfsr_lucasKanadeSweepBatch(m, fr, (const float*)ref.pyr[0].ptr, L.flowBuf[0].pitch, ref.pyr[0].pitch, L.work[0].lkSum[0].pitch,
                                       L.tw, L.th, c.lkHalfWindow, c.lkMinDet, lastIt ? (float)L.flowScale : 1.0f, stream));
        b->paths[MFSR_PATH_LK_SWEEP_BATCH]++;
    }
    // robustness masks
    bool maskBatch = stageBatch && m > 0;
    if (maskBatch && maskGroup) {
        mfsr_robustness_group_frame gf[MFSR_MAX_FUSE_GROUP];
        for (int k = 0; k < m; k++) {
            const int slot = g.slot[idx[mq[k]]];
            gf[k].movedMeans = (const mfsr_float3*)L.mov[mq[k]].half.ptr;
            gf[k].movedRaw = g.raw[idx[mq[k]]];
            gf[k].mask = (mfsr_float4*)(c.maskErode > 0 ? L.maskRaw[k].ptr : L.maskBuf[slot].ptr);
            gf[k].flow = (const mfsr_float2*)final_flow(b, slot, 0)->ptr;
        }
        TRY(mfsr_cfa::robustnessMaskGroup(b->cfa, m, gf, (const mfsr_float3*)ref.half.ptr, ref.half.pitch, L.flowBuf[0].pitch, L.mov[0].half.pitch,
                                     L.maskBuf[0].pitch, L.hw, L.hh, c.maxVal, c.alpha, c.beta, c.thresholdM, stream));
        b->robustGroupLaunches++;
        b->paths[MFSR_PATH_ROBUST_BATCH]++;
    } else if (maskBatch) {
        mfsr_robustness_frame rf[MFSR_MAX_FUSE_GROUP];
        for (int k = 0; k < m; k++) {
            const int slot = g.slot[idx[mq[k]]];
            rf[k].movedHalf = (const mfsr_float3*)L.mov[mq[k]].half.ptr;
            rf[k].mask = (mfsr_float4*)(c.maskErode > 0 ? L.maskRaw[k].ptr : L.maskBuf[slot].ptr);
            rf[k].flow = (const mfsr_float2*)final_flow(b, slot, 0)->ptr;
        }
        const int rc = mfsr_robustnessMaskFusedBatch(m, rf, (const mfsr_float3*)ref.half.ptr, L.flowBuf[0].pitch, L.tw, L.th, L.hw, L.hh,
                                                     ref.half.pitch, L.maskBuf[0].pitch, c.alpha, c.beta, c.thresholdM, stream);
        if (rc == MFSR_E_UNSUPPORTED)
            maskBatch = false;  // (the straight robustness kernel was selected: frame by frame below)
        else if (rc)
            return rc;
        else
            b->paths[MFSR_PATH_ROBUST_BATCH]++;
    }
    if (maskBatch && c.maskErode > 0) {  // one erosion launch for the whole group
        const mfsr_float4* ein[MFSR_MAX_FUSE_GROUP];
        mfsr_float4* eout[MFSR_MAX_FUSE_GROUP];
        for (int k = 0; k < m; k++) {
            ein[k] = (const mfsr_float4*)L.maskRaw[k].ptr;
            eout[k] = (mfsr_float4*)L.maskBuf[g.slot[idx[mq[k]]]].ptr;
        }
        TRY(mfsr_erodeMaskBatch(m, ein, eout, L.hw, L.hh, L.maskRaw[0].pitch, L.maskBuf[0].pitch, c.maskErode, stream));
    }
    for (int q = 0; q < n; q++) {
        const int i = idx[q], slot = g.slot[i];
        if (!g.isRef[i] && !maskBatch) TRY(align_post(b, slot, L.mov[q], stream));
        aligned_outputs(b, slot, g.isRef[i], &g.flow[i], &g.mask[i]);
        g.deferred[i] = false;
        b->flowCur = g.flow[i];
        b->maskCur = g.mask[i];
        if (b->fuseStream) MFSR_HIP_TRY(hipEventRecord(b->evAligned[g.slot[i]], mfsr_s(stream)));
    }
    return MFSR_OK;
}

// hostBurst: the frame belongs to a host-frame burst (mfsr_burst_add_frame_host), whose last groups wait for
// mfsr_burst_finish_host; a frame added through mfsr_burst_add_frame never leaves a complete group waiting
// prepared / suppliedShifts: the frame's products and its tile shifts where the caller has made them (frame streams, joint mode)
static int add_frame_impl(mfsr_burst* b, const uint16_t* raw, int isReference, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                          bool hostBurst, mfsr_stream_t stream, const FrameProducts* prepared = nullptr,
                          const Img* suppliedShifts = nullptr)
{
    MFSR_REQUIRE(b && raw && imgOut && totalWeights);
    MFSR_REQUIRE(b->haveRef);
    MFSR_REQUIRE(!b->refStale);  // after mfsr_burst_process_joint: call mfsr_burst_set_reference first
    const mfsr_config& c = b->cfg;
    b->holdLastGroup = hostBurst;
    // G: accumulate onto the HR grid -- alone, or together with the frames that were waiting for the rest of their group
    if (b->pend.n && (b->pend.imgOut != imgOut || b->pend.totalWeights != totalWeights)) TRY(flush_pending(b, stream));
    // burst hold: held groups leave when this frame goes to other accumulators, or when its ring slot would be one of theirs
    if (b->nHold && (b->hold[0].imgOut != imgOut || b->hold[0].totalWeights != totalWeights ||
                     b->nHold * MFSR_MAX_FUSE_GROUP + b->pend.n >= b->ring))
        TRY(drain_waiting(b, stream, false));
    // a complete group was held back for mfsr_burst_finish_host and frames keep arriving (more than cfg.frames per
    // reference, or a resident frame after a host burst): it is fused the ordinary way before this frame is registered
    if (b->pend.n >= b->group) TRY(accumulate_pending(b, stream));
    MFSR_REQUIRE(b->pend.n < MFSR_MAX_FUSE_GROUP);
    const int slot = b->frameCounter++ % b->ring;
    const Img *flow = nullptr, *mask = nullptr;
    const bool defer = can_defer_alignment(b, prepared || suppliedShifts);
    b->paths[defer ? MFSR_PATH_FRAMES_DEFERRED : MFSR_PATH_FRAMES_IMMEDIATE]++;
    if (!defer) {
        TRY(align_deferred(b, b->pend, stream));  // keep the alignment in frame order on the stream
        TRY(align_frame(b, raw, isReference, slot, prepared, suppliedShifts, &flow, &mask, stream));
        b->flowCur = flow;
        b->maskCur = mask;
        if (b->fuseStream) MFSR_HIP_TRY(hipEventRecord(b->evAligned[slot], mfsr_s(stream)));
    }
    if (defer) b->slotFlow[slot] = nullptr;  // (mfsr_burst_debug_frame_views: not aligned yet)
    const int i = b->pend.n++;
    b->pend.slot[i] = slot;
    b->pend.raw[i] = raw;
    b->pend.flow[i] = flow;
    b->pend.mask[i] = mask;
    b->pend.deferred[i] = defer;
    b->pend.isRef[i] = isReference;
    b->pend.imgOut = imgOut;
    b->pend.totalWeights = totalWeights;
    b->framesSinceRef++;
    if (b->pend.n < b->group) return MFSR_OK;  // the group is fused when its last frame arrives (or on flush / finish)
    // host bursts: the group that the burst's last frame completes is fused band by band by mfsr_burst_finish_host, so that
    // finished bands of the image leave for the host while the later ones are still being fused
    // (only the group the burst's LAST frame completes: frames beyond cfg.frames are fused as they come)
    if (b->holdLastGroup && b->framesSinceRef == c.frames) return MFSR_OK;
    // ... and so does the group before it (MFSR_HOST_HOLD=2, the default): the first band of the image is then complete after
    // 1/8 of two groups' fuse instead of after a whole group's, and the download -- the tail of the burst -- starts that much
    // earlier; the earlier groups are fused as they arrive, under the uploads
    static const int holdGroups = mfsr_env_int("MFSR_HOST_HOLD", 2);
    if (b->holdLastGroup && holdGroups >= 2 && !b->heldHas && c.frames - b->framesSinceRef <= b->group &&
        c.frames - b->framesSinceRef > 0 && !b->pend.deferred[0]) {
        bool aligned = true;
        for (int j = 0; j < b->pend.n; j++) aligned = aligned && !b->pend.deferred[j];
        if (aligned) {
            b->held = b->pend;
            b->heldHas = true;
            b->pend.n = 0;
            return MFSR_OK;
        }
    }
    // burst hold (mfsr_burst_hold_fuse): the group is aligned now, as always, and its fuse waits for the burst launch
    if (can_hold_group(b, hostBurst)) {
        TRY(align_deferred(b, b->pend, stream));
        b->hold[b->nHold++] = b->pend;
        b->pend.n = 0;
        return MFSR_OK;
    }
    return accumulate_pending(b, stream);
}

extern "C" int mfsr_burst_add_frame(mfsr_burst* b, const uint16_t* raw, int isReference, mfsr_float3* imgOut,
                                    mfsr_float3* totalWeights, mfsr_stream_t stream)
{
    return add_frame_impl(b, raw, isReference, imgOut, totalWeights, false, stream);
}

extern "C" int mfsr_burst_group_size(const mfsr_config* cfg)
{
    if (!cfg || cfg->pairFrames <= 0) return 1;
    if (cfg->pairFrames >= 2) return cfg->pairFrames < MFSR_MAX_FUSE_GROUP ? cfg->pairFrames : MFSR_MAX_FUSE_GROUP;
    // as many as one launch takes: the x2 and x4 Bayer tile kernels fuse four, every other geometry two
    return ((cfg->scale == 2 || cfg->scale == 4) && !cfg->mono) ? MFSR_MAX_FUSE_GROUP : 2;
}

// ---- building blocks of stripe-sharded bursts (multi-GPU: frames are aligned where they live, every rank fuses ALL
//      frames onto its own stripe of HR rows; csrc/dist.cpp and the Python mirror drive these) -----------------------
extern "C" int mfsr_burst_field_dims(const mfsr_burst* b, int* flowW, int* flowH, int* maskW, int* maskH)
{
    MFSR_REQUIRE(b != nullptr);
    if (flowW) *flowW = b->L.tw;
    if (flowH) *flowH = b->L.th;
    if (maskW) *maskW = b->L.hw;
    if (maskH) *maskH = b->L.hh;
    return MFSR_OK;
}

extern "C" int mfsr_burst_align_frame(mfsr_burst* b, const uint16_t* raw, int isReference, mfsr_float2* flowOut, int flowPitch,
                                      mfsr_float4* maskOut, int maskPitch, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && raw && flowOut && maskOut);
    MFSR_REQUIRE(b->haveRef);
    MFSR_REQUIRE(!b->refStale);  // after mfsr_burst_process_joint: call mfsr_burst_set_reference first
    const Layout& L = b->L;
    MFSR_REQUIRE((long long)flowPitch >= 8LL * L.tw && (flowPitch & 7) == 0 && ((uintptr_t)flowOut & 7) == 0);
    MFSR_REQUIRE((long long)maskPitch >= 16LL * L.hw && (maskPitch & 15) == 0 && ((uintptr_t)maskOut & 15) == 0);
    TRY(drain_waiting(b, stream, false));  // (the call takes a ring slot)
    const int slot = b->frameCounter++ % b->ring;
    const Img *flow = nullptr, *mask = nullptr;
    TRY(align_frame(b, raw, isReference, slot, nullptr, nullptr, &flow, &mask, stream));
    b->flowCur = flow;
    b->maskCur = mask;
    MFSR_HIP_TRY(hipMemcpy2DAsync(flowOut, flowPitch, flow->ptr, flow->pitch, (size_t)L.tw * 8, L.th, hipMemcpyDeviceToDevice,
                                  mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemcpy2DAsync(maskOut, maskPitch, mask->ptr, mask->pitch, (size_t)L.hw * 16, L.hh, hipMemcpyDeviceToDevice,
                                  mfsr_s(stream)));
    return MFSR_OK;
}

// mfsr_burst_align_frame for several frames: groups of up to mfsr_burst_group_size frames are aligned as one batch (the
// launches of mfsr_burst_add_frame's groups: a frame's result does not depend on the batch it is in)
extern "C" int mfsr_burst_align_frames(mfsr_burst* b, int nFrames, const uint16_t* const* raws, const int* isReference,
                                       mfsr_float2* const* flowOut, int flowPitch, mfsr_float4* const* maskOut, int maskPitch,
                                       mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && raws && flowOut && maskOut && nFrames >= 0);
    MFSR_REQUIRE(b->haveRef && !b->refStale);
    MFSR_REQUIRE(b->pend.n == 0);  // no frame of an add_frame group may be waiting
    const Layout& L = b->L;
    MFSR_REQUIRE((long long)flowPitch >= 8LL * L.tw && (flowPitch & 7) == 0);
    MFSR_REQUIRE((long long)maskPitch >= 16LL * L.hw && (maskPitch & 15) == 0);
    for (int k = 0; k < nFrames; k++)
        MFSR_REQUIRE(raws[k] && flowOut[k] && maskOut[k] && ((uintptr_t)flowOut[k] & 7) == 0 && ((uintptr_t)maskOut[k] & 15) == 0);
    TRY(drain_waiting(b, stream, false));  // (the call takes ring slots)
    const bool batch = can_defer_alignment(b, false);
    const int per = batch ? b->group : 1;
    for (int k0 = 0; k0 < nFrames; k0 += per) {
        const int n = nFrames - k0 < per ? nFrames - k0 : per;
        FuseGroup p = {};  // (these frames are not waiting for a fuse: the group lives for this batch only)
        p.n = n;
        for (int j = 0; j < n; j++) {
            p.slot[j] = b->frameCounter++ % b->ring;
            p.raw[j] = raws[k0 + j];
            p.isRef[j] = isReference ? isReference[k0 + j] : 0;
            p.deferred[j] = batch;
            if (!batch) TRY(align_frame(b, p.raw[j], p.isRef[j], p.slot[j], nullptr, nullptr, &p.flow[j], &p.mask[j], stream));
        }
        TRY(align_deferred(b, p, stream));
        for (int j = 0; j < n; j++) {
            b->flowCur = p.flow[j];
            b->maskCur = p.mask[j];
            MFSR_HIP_TRY(hipMemcpy2DAsync(flowOut[k0 + j], flowPitch, p.flow[j]->ptr, p.flow[j]->pitch, (size_t)L.tw * 8, L.th,
                                          hipMemcpyDeviceToDevice, mfsr_s(stream)));
            MFSR_HIP_TRY(hipMemcpy2DAsync(maskOut[k0 + j], maskPitch, p.mask[j]->ptr, p.mask[j]->pitch, (size_t)L.hw * 16, L.hh,
                                          hipMemcpyDeviceToDevice, mfsr_s(stream)));
        }
    }
    return MFSR_OK;
}

extern "C" int mfsr_burst_fuse_rows(mfsr_burst* b, int nFrames, const uint16_t* const* raws, const mfsr_float2* const* flows,
                                    int flowPitch, const mfsr_float4* const* masks, int maskPitch, mfsr_float3* imgOut,
                                    mfsr_float3* totalWeights, int accumulatorsUndefined, int rowBegin, int rowEnd,
                                    mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && raws && flows && masks && imgOut && totalWeights && nFrames >= 1 && nFrames <= MFSR_MAX_FUSE_GROUP);
    MFSR_REQUIRE(b->haveRef && !b->win.on);  // (row stripes of whole-frame accumulators)
    TRY(wait_ref_products(b, stream));
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    const mfsr_float3 white = cfg_white(c), black = cfg_black(c);
    mfsr_tex2d sh[MFSR_MAX_FUSE_GROUP];
    for (int n = 0; n < nFrames; n++) {
        sh[n].ptr = flows[n];
        sh[n].pitch = flowPitch;
        sh[n].width = L.tw;
        sh[n].height = L.th;
    }
    bool timed;
    TRY(timed_begin(b, stream, &timed));
    TRY(mfsr_cfa::accumulateSuperResFullRows(b->cfa, nFrames, raws, imgOut, totalWeights, masks, as_tex(L.kparam4), sh, white, black, L.W, L.H,
                                        c.scale, 12 * L.hrW, maskPitch, accumulatorsUndefined, rowBegin, rowEnd, stream));
    return timed_end(b, timed, 1, nFrames, stream);
}

// Stripe plan of rank `rank` of `worldSize`: its HR rows and the rows of every per-frame product its fuse reads.
// Pure host arithmetic (no device), shared by csrc/dist.cpp and the Python mirror so that both exchange the same rows.
extern "C" int mfsr_dist_stripe_plan(const mfsr_config* cfg, int worldSize, int rank, int rawHalo, mfsr_stripe_plan* out)
{
    MFSR_REQUIRE(out != nullptr && worldSize >= 1 && rank >= 0 && rank < worldSize && rawHalo >= 4);
    TRY(validate(cfg));
    const int s = cfg->scale, W = cfg->width, H = cfg->height;
    const int hrH = s * H;
    const int th = cfg->mono ? H : H / 2, hh = H / 2;
    (void)W;
    // stripes start on multiples of 16 HR rows (tile rows of every fuse kernel, mfsr_accumulateSuperResFullRows)
    auto cut = [&](int g) { return g >= worldSize ? hrH : (int)((long long)hrH * g / worldSize / 16 * 16); };
    const int r0 = cut(rank), r1 = cut(rank + 1);
    memset(out, 0, sizeof(*out));
    out->rowBegin = r0;
    out->rowEnd = r1;
    if (r1 <= r0) return MFSR_OK;  // more ranks than 16-row bands: this rank fuses nothing
    // a field with fh rows is sampled at HR row Y through rows floor((Y + .5) * fh / hrH - .5) and the next one
    auto rows_of = [&](int fh, int pad, int* first, int* count) {
        const int per = hrH / fh;  // HR rows per field row (exact: validate() makes H a multiple of 4)
        int a = r0 / per - 1 - pad, b = (r1 + per - 1) / per + 1 + pad;
        if (a < 0) a = 0;
        if (b > fh) b = fh;
        *first = a;
        *count = b - a;
    };
    rows_of(th, 0, &out->flowRow0, &out->flowRows);
    rows_of(hh, 1, &out->maskRow0, &out->maskRows);  // + the 5x5 footprint: site (Y + py) / s / 2, |py| <= 2
    {
        int a = r0 / s - rawHalo, b = (r1 + s - 1) / s + rawHalo;  // raw row (Y + py + round(s * v)) / s: |v| <= rawHalo - 3
        if (a < 0) a = 0;
        if (b > H) b = H;
        out->rawRow0 = a;
        out->rawRows = b - a;
    }
    out->maxFlowY = (float)(rawHalo - 3);
    return MFSR_OK;
}

extern "C" int mfsr_burst_begin(mfsr_burst* b, mfsr_float3* imgOut, mfsr_float3* totalWeights, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && imgOut && totalWeights);
    TRY(flush_pending(b, stream));  // whatever was still waiting belongs to the previous burst
    memset(b->paths, 0, sizeof(b->paths));
    b->sharpenedFinishes = b->denoisedFinishes = b->chainedFinishes = b->geometryFinishes = 0;
    b->robustGroupLaunches = 0;
    b->fusedFinishes = 0;
    b->burstLaunches = b->burstGroups = 0;
    b->fresh.has = true;
    b->fresh.imgOut = imgOut;
    b->fresh.totalWeights = totalWeights;
    return MFSR_OK;
}

extern "C" int mfsr_burst_flush(mfsr_burst* b, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b != nullptr);
    return flush_pending(b, stream);
}

// ---- rendered output ---------------------------------------------------------------------------------
// bytes of a dense row of the burst's integer output: rendered bytes of the format, or uint16_t RGB
static size_t out_row_bytes(const mfsr_burst* b)
{
    return b->renderOn ? (size_t)mfsr_render_row_bytes(b->render.format, out_w(b)) : (size_t)out_w(b) * 6;
}

// a two-plane 4:2:0 format (yuv_format, render_common.hpp): the output buffer holds out_h rows of Y, then
// out_h / 2 rows of chroma, one pitch
static bool yuv_on(const mfsr_burst* b) { return b->renderOn && yuv_format(b->render.format); }

// bytes of the burst's dense integer output
static size_t out_image_bytes(const mfsr_burst* b)
{
    return b->renderOn ? (size_t)mfsr_render_image_bytes(b->render.format, out_w(b), out_h(b)) : (size_t)out_w(b) * 6 * out_h(b);
}

// A finish with a reach: a stencil on the value the finish holds -- the sharpened (§2.20) or the denoised (§2.24) finish, never
// both, or a chain (§2.26) with one of those stages or both -- reads R rows beyond the rows it writes.
static bool stencil_on(const mfsr_burst* b) { return b->sharpenOn || b->denoiseOn || (b->chainOn && b->chainReach > 0); }

// Rows [r0, r0 + rows) of the burst's accumulators (of its window's, when one is set) as a finish launch or a statistics pass
// takes them; imgOut and totalWeights are the whole images.
struct FinishView {
    const mfsr_float3 *acc, *wt;  // the first pixel of row r0
    size_t off;                   // its bytes into the accumulators, and into a float output image
    int pitch, w, rows;
    int x0, y0;                   // the pixel of the full HR frame that the view's pixel (0, 0) is
};

static FinishView finish_view(const mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, int r0, int rows)
{
    FinishView v;
    v.w = out_w(b);
    v.rows = rows;
    v.pitch = 12 * v.w;
    v.off = (size_t)r0 * v.pitch;
    v.acc = (const mfsr_float3*)((const char*)imgOut + v.off);
    v.wt = (const mfsr_float3*)((const char*)totalWeights + v.off);
    v.x0 = b->win.on ? b->win.x0 : 0;
    v.y0 = (b->win.on ? b->win.y0 : 0) + r0;
    return v;
}

// the arguments every finish entry point begins with (the accumulator pair, the fallback: the whole LR image) and the four that
// place the view in the full frame
#define FINISH_SOURCE(b, v) \
    (v).acc, (v).wt, (v).pitch, (const mfsr_float3*)(b)->L.fallback.ptr, (b)->L.fallback.pitch, (b)->L.W, (b)->L.H, 0.0f, 1.0f, 0.0f, 1.0f
#define FINISH_PLACE(b, v) (v).x0, (v).y0, (b)->L.hrW, (b)->L.hrH

// The finish of output rows [r0, r0 + rows) (rows of the window when one is set) in one launch on the accumulators, whatever the
// burst is set to.  Pointers are those of the whole images; `out` holds dense rows of the integer output: uint16_t RGB, or the
// render description's format (two-plane formats: both planes, so r0 and rows are even).  A stencil finish reads rowsAbove /
// rowsBelow rows beyond its own (stencil_reach), which are complete; the pointwise finishes take 0, 0.
static int finish_rows(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, mfsr_float3* outImg, void* out,
                       int r0, int rows, int rowsAbove, int rowsBelow, mfsr_stream_t stream)
{
    const mfsr_config& c = b->cfg;
    const FinishView v = finish_view(b, imgOut, totalWeights, r0, rows);
    const int rowBytes = (int)out_row_bytes(b);
    mfsr_float3* outF = outImg ? (mfsr_float3*)((char*)outImg + v.off) : nullptr;
    char* outQ = out ? (char*)out + (size_t)r0 * rowBytes : nullptr;
    const mfsr_render* render = b->renderOn ? &b->render : nullptr;  // (none: the stencil entries render plainly themselves)
    // A chain (§2.26) takes every finish of the burst, whatever the format: the setters keep it apart from the three below.
    if (b->chainOn) {
        const bool yuv = yuv_on(b);
        if (yuv) MFSR_REQUIRE((v.w & 1) == 0 && (out_h(b) & 1) == 0 && (r0 & 1) == 0 && (rows & 1) == 0);
        char* uv = yuv && out ? (char*)out + ((size_t)out_h(b) + (size_t)(r0 / 2)) * rowBytes : nullptr;
        b->chainedFinishes++;
        return mfsr_finishChain(FINISH_SOURCE(b, v), outF, v.pitch, outQ, rowBytes, uv, rowBytes, render, v.w, rows, c.weightThreshold,
                                c.applyGamma, FINISH_PLACE(b, v), &b->chain, b->chainGrid, rowsAbove, rowsBelow, stream);
    }
    // Which launch: denoised, sharpened, two-plane, local tone, rendered, plain.  The setters (mfsr_burst_set_sharpen, _denoise,
    // _render, _local_tone: whichever comes second is refused) leave at most one of the first four on: never two stencils, no
    // stencil with a two-plane format or with local tone, no local tone with a two-plane format -- and none with a host burst
    // (cfg.uploadRing), whose bands therefore never meet it.  So the order of the first four decides nothing.
    if (b->denoiseOn) {
        b->denoisedFinishes++;
        return mfsr_finishDenoised(FINISH_SOURCE(b, v), outF, v.pitch, outQ, rowBytes, render, v.w, rows, c.weightThreshold, c.applyGamma,
                                   FINISH_PLACE(b, v), &b->denoise, rowsAbove, rowsBelow, stream);
    }
    if (b->sharpenOn) {
        b->sharpenedFinishes++;
        return mfsr_finishSharpened(FINISH_SOURCE(b, v), outF, v.pitch, outQ, rowBytes, render, v.w, rows, c.weightThreshold, c.applyGamma,
                                    FINISH_PLACE(b, v), &b->sharpen, rowsAbove, rowsBelow, stream);
    }
    if (yuv_on(b)) {
        MFSR_REQUIRE((v.w & 1) == 0 && (out_h(b) & 1) == 0 && (r0 & 1) == 0 && (rows & 1) == 0);
        char* uv = out ? (char*)out + ((size_t)out_h(b) + (size_t)(r0 / 2)) * rowBytes : nullptr;
        return mfsr_finishRenderedYuv(FINISH_SOURCE(b, v), outF, v.pitch, outQ, rowBytes, uv, rowBytes, render, v.w, rows,
                                      c.weightThreshold, c.applyGamma, FINISH_PLACE(b, v), stream);
    }
    if (b->localToneOn) {  // (§2.25; without a render description: uint16_t RGB of the gained linear image)
        const mfsr_render plain = mfsr_plain_render();
        return mfsr_finishLocalTone(FINISH_SOURCE(b, v), outF, v.pitch, outQ, rowBytes, render ? render : &plain, v.w, rows,
                                    c.weightThreshold, c.applyGamma, FINISH_PLACE(b, v), b->localToneGrid, &b->localTone, stream);
    }
    if (render)
        return mfsr_finishRendered(FINISH_SOURCE(b, v), outF, v.pitch, outQ, rowBytes, render, v.w, rows, c.weightThreshold, c.applyGamma,
                                   FINISH_PLACE(b, v), stream);
    return mfsr_finishFusedWindow(FINISH_SOURCE(b, v), outF, v.pitch, (uint16_t*)outQ, v.w, rows, c.weightThreshold, c.applyGamma,
                                  65535.0f, FINISH_PLACE(b, v), stream);
}

// rows of the output above / below [r0, r0 + rows) that a stencil finish of those rows reads
static void stencil_reach(const mfsr_burst* b, int r0, int rows, int* above, int* below)
{
    const int R = b->chainOn ? b->chainReach : (b->denoiseOn ? b->denoise.radius : b->sharpen.radius), rest = out_h(b) - r0 - rows;
    *above = R < r0 ? R : r0;
    *below = R < rest ? R : rest;
}

extern "C" int mfsr_burst_set_sharpen(mfsr_burst* b, const mfsr_sharpen* sharpen)
{
    MFSR_REQUIRE(b != nullptr);
    MFSR_REQUIRE(burst_idle(b));  // between bursts only
    if (!sharpen) {
        b->sharpenOn = false;
        return MFSR_OK;
    }
    TRY(mfsr_sharpen_validate(sharpen));
    const bool on = sharpen_on(sharpen);
    MFSR_REQUIRE(!(on && yuv_on(b)));  // the sharpen tile kernel renders single rows: no two-plane output
    MFSR_REQUIRE(!(on && b->denoiseOn));  // one stencil per finish: whichever setter comes second is refused
    MFSR_REQUIRE(!(on && b->localToneOn));  // the local-tone finish is pointwise: no stencil
    MFSR_REQUIRE(!(on && b->chainOn));      // a chain is installed: its own sharpen stage is the way
    b->sharpen = *sharpen;
    b->sharpenOn = on;
    return MFSR_OK;
}

extern "C" int mfsr_burst_set_denoise(mfsr_burst* b, const mfsr_denoise* denoise)
{
    MFSR_REQUIRE(b != nullptr);
    MFSR_REQUIRE(burst_idle(b));  // between bursts only
    if (!denoise) {
        b->denoiseOn = false;
        return MFSR_OK;
    }
    TRY(mfsr_denoise_validate(denoise));
    const bool on = denoise_on(denoise);
    MFSR_REQUIRE(!(on && yuv_on(b)));     // the denoise tile kernel renders single rows, as the sharpen one
    MFSR_REQUIRE(!(on && b->sharpenOn));  // one stencil per finish
    MFSR_REQUIRE(!(on && b->localToneOn));  // (as mfsr_burst_set_sharpen)
    MFSR_REQUIRE(!(on && b->chainOn));      // (likewise)
    b->denoise = *denoise;
    b->denoiseOn = on;
    return MFSR_OK;
}

extern "C" int mfsr_burst_debug_denoised(const mfsr_burst* b, int* finishes)
{
    MFSR_REQUIRE(b && finishes);
    *finishes = b->denoisedFinishes;
    return MFSR_OK;
}

// ---- the finish chain -------------------------------------------------------------------------------
extern "C" int mfsr_burst_set_finish_chain(mfsr_burst* b, const mfsr_finish_chain* chain, const float* gridDev)
{
    MFSR_REQUIRE(b != nullptr);
    MFSR_REQUIRE(burst_idle(b));  // between bursts only
    int reach = 0;
    if (chain) TRY(mfsr_finish_chain_reach(chain, &reach));  // (validates)
    if (!chain || (reach == 0 && !chain->useLocalTone)) {    // every stage off: no chain
        b->chainOn = false;
        b->chainGrid = nullptr;
        b->chainReach = 0;
        return MFSR_OK;
    }
    MFSR_REQUIRE(!b->sharpenOn && !b->denoiseOn && !b->localToneOn);  // one way to each stage: the chain's, or the setter's
    MFSR_REQUIRE((gridDev != nullptr) == (chain->useLocalTone != 0) && ((uintptr_t)gridDev & 3) == 0);
    MFSR_REQUIRE(!(chain->useLocalTone && b->cfg.uploadRing));  // a host burst finishes band by band: no grid can be measured first
    b->chain = *chain;
    b->chainGrid = gridDev;
    b->chainReach = reach;
    b->chainOn = true;
    return MFSR_OK;
}

extern "C" int mfsr_burst_debug_chained(const mfsr_burst* b, int* finishes)
{
    MFSR_REQUIRE(b && finishes);
    *finishes = b->chainedFinishes;
    return MFSR_OK;
}

extern "C" int mfsr_burst_debug_robust_group(const mfsr_burst* b, int* launches)
{
    MFSR_REQUIRE(b && launches);
    *launches = b->robustGroupLaunches;
    return MFSR_OK;
}

extern "C" int mfsr_burst_debug_sharpened(const mfsr_burst* b, int* finishes)
{
    MFSR_REQUIRE(b && finishes);
    *finishes = b->sharpenedFinishes;
    return MFSR_OK;
}

extern "C" int mfsr_burst_set_render(mfsr_burst* b, const mfsr_render* render)
{
    MFSR_REQUIRE(b != nullptr);
    MFSR_REQUIRE(burst_idle(b));  // between bursts only
    if (!render) {
        b->renderOn = false;
        return MFSR_OK;
    }
    TRY(mfsr_render_validate(render));
    // (as mfsr_burst_set_sharpen / _denoise: whichever comes second; a chain, §2.26, stores the two-plane formats itself)
    MFSR_REQUIRE(!((b->sharpenOn || b->denoiseOn) && yuv_format(render->format)));
    MFSR_REQUIRE(!(b->localToneOn && yuv_format(render->format)));  // (mfsr_burst_set_local_tone likewise)
    b->render = *render;
    b->renderOn = true;
    return MFSR_OK;
}

// ---- auto white balance and auto tone: the accumulators measured with the finish's own arguments
//      (csrc/image_stats.hip), the fits on the host, the result installed as the burst's render description ---------------------
// one measurement of the burst's output (or window) into the zeroed table, downloaded into b->autoStats; waits for the stream
static int auto_measure(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, const mfsr_image_stats_params* p,
                        uint64_t* statsDev, mfsr_stream_t stream)
{
    const FinishView v = finish_view(b, imgOut, totalWeights, 0, out_h(b));
    MFSR_HIP_TRY(hipMemsetAsync(statsDev, 0, sizeof(uint64_t) * MFSR_IMAGE_STATS_WORDS, mfsr_s(stream)));
    TRY(mfsr_finishStats(FINISH_SOURCE(b, v), v.w, v.rows, b->cfg.weightThreshold, FINISH_PLACE(b, v), p, statsDev, stream));
    b->autoStats.resize(MFSR_IMAGE_STATS_WORDS);
    MFSR_HIP_TRY(hipMemcpyAsync(b->autoStats.data(), statsDev, sizeof(uint64_t) * MFSR_IMAGE_STATS_WORDS, hipMemcpyDeviceToHost,
                                mfsr_s(stream)));
    MFSR_HIP_TRY(hipStreamSynchronize(mfsr_s(stream)));
    return MFSR_OK;
}

extern "C" int mfsr_burst_auto_render(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights,
                                      const mfsr_auto_params* apIn, uint64_t* statsDev, float* lutDev, mfsr_render* render,
                                      mfsr_auto_result* res, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && imgOut && totalWeights && statsDev && render && res);
    MFSR_REQUIRE(b->haveRef && ((uintptr_t)statsDev & 7) == 0);
    MFSR_REQUIRE(!b->cfg.uploadRing);  // a host burst finishes band by band, before its accumulators are complete
    const long long pixels = (long long)out_w(b) * out_h(b);
    mfsr_auto_params ap;
    if (apIn)
        ap = *apIn;
    else
        TRY(mfsr_auto_defaults(pixels, &ap));
    MFSR_REQUIRE(ap.iterations >= 1 && ap.iterations <= 4 && ap.toneSize >= 1 && ap.toneSize <= 65536);
    MFSR_REQUIRE(0 <= ap.lo && ap.lo <= ap.hi && ap.hi <= MFSR_IMAGE_STATS_BINS - 1 && 0 <= ap.chromaTol && ap.chromaTol <= 65536);
    MFSR_REQUIRE(ap.reserved[0] == 0 && ap.reserved[1] == 0 && ap.reserved[2] == 0);
    if (ap.tone) MFSR_REQUIRE(lutDev != nullptr && ((uintptr_t)lutDev & 3) == 0);
    TRY(mfsr_render_validate(render));  // (before any work: the format, the caller's matrix and table)
    TRY(flush_pending(b, stream));
    const long long minCount = ap.minCount > 0 ? ap.minCount : pixels / 64;

    mfsr_auto_result out;
    memset(&out, 0, sizeof(out));
    out.gains[0] = out.gains[1] = out.gains[2] = 1.0f;
    out.white = out.gamma = 1.0;
    mfsr_image_stats_params sp;
    memset(&sp, 0, sizeof(sp));
    sp.lo = ap.lo;
    sp.hi = ap.hi;
    if (ap.awb) {
        float g[3] = {1.0f, 1.0f, 1.0f};
        for (int pass = 0; pass < ap.iterations; pass++) {
            sp.useMatrix = pass > 0;
            sp.chromaTol = pass > 0 ? ap.chromaTol : 0;
            for (int k = 0; k < 3; k++) sp.matrix[4 * k] = g[k];
            TRY(auto_measure(b, imgOut, totalWeights, &sp, statsDev, stream));
            const uint64_t* t = b->autoStats.data();
            out.neutralShare = t[0] ? (double)t[1] / (double)t[0] : 0.0;
            float c[3];
            int32_t st = 0;
            TRY(mfsr_awb_gains(t, minCount, c, &st));
            if (st == 1) {
                if (pass == 0) out.awbStatus = 1;
                continue;  // (this pass leaves g as it is)
            }
            if (st == 2 && out.awbStatus == 0) out.awbStatus = 2;
            for (int k = 0; k < 3; k++) {
                double v = (double)g[k] * (double)c[k];
                if (v < 0.125 || v > 8.0) {
                    v = v < 0.125 ? 0.125 : 8.0;
                    if (out.awbStatus == 0) out.awbStatus = 2;
                }
                g[k] = (float)v;
            }
            out.awbPasses++;
        }
        for (int k = 0; k < 3; k++) out.gains[k] = g[k];
        float m[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double ccm = render->useMatrix ? (double)render->matrix[3 * i + j] : (i == j ? 1.0 : 0.0);
                m[3 * i + j] = (float)(ccm * (double)g[j]);
                MFSR_REQUIRE(fabsf(m[3 * i + j]) <= 256.0f);
            }
        memcpy(render->matrix, m, sizeof(m));
        render->useMatrix = 1;
    }
    if (ap.tone) {
        memset(&sp, 0, sizeof(sp));
        sp.lo = ap.lo;
        sp.hi = ap.hi;
        sp.useMatrix = render->useMatrix != 0;
        memcpy(sp.matrix, render->matrix, sizeof(sp.matrix));
        TRY(auto_measure(b, imgOut, totalWeights, &sp, statsDev, stream));
        b->autoLut.resize((size_t)ap.toneSize + 1);
        TRY(mfsr_tone_fit(b->autoStats.data(), &ap.toneParams, ap.toneSize, b->autoLut.data(), &out.black, &out.white, &out.gamma,
                          &out.toneStatus));
        MFSR_HIP_TRY(hipMemcpyAsync(lutDev, b->autoLut.data(), sizeof(float) * b->autoLut.size(), hipMemcpyHostToDevice, mfsr_s(stream)));
        MFSR_HIP_TRY(hipStreamSynchronize(mfsr_s(stream)));  // (the staging may be written again by the next call)
        render->toneLut = lutDev;
        render->toneSize = ap.toneSize;
    }
    TRY(mfsr_burst_set_render(b, render));  // (after the flush its own guard holds)
    *res = out;
    return MFSR_OK;
}

// ---- local tone mapping in the finish: the grid of the full HR frame, measured on the accumulators with the
//      finish's own arguments (csrc/local_tone.hip), fitted on the host, installed for finish_rows ------------------------------
extern "C" int mfsr_burst_set_local_tone(mfsr_burst* b, const mfsr_local_tone* lt, const float* gridDev)
{
    MFSR_REQUIRE(b != nullptr);
    MFSR_REQUIRE(burst_idle(b));  // between bursts only
    if (!lt) {
        b->localToneOn = false;
        b->localToneGrid = nullptr;
        return MFSR_OK;
    }
    TRY(mfsr_local_tone_validate(lt));
    MFSR_REQUIRE(gridDev != nullptr && ((uintptr_t)gridDev & 3) == 0);
    MFSR_REQUIRE(!b->cfg.uploadRing);  // a host burst finishes band by band, before its accumulators are complete
    MFSR_REQUIRE(!stencil_on(b));      // whichever setter comes second is refused
    MFSR_REQUIRE(!b->chainOn);         // (a chain, §2.26, takes its grid with its own setter)
    MFSR_REQUIRE(!yuv_on(b));          // single-plane formats only
    b->localTone = *lt;
    b->localToneGrid = gridDev;
    b->localToneOn = true;
    return MFSR_OK;
}

extern "C" int mfsr_burst_local_tone(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights,
                                     const mfsr_local_tone* ltIn, uint64_t* statsDev, float* gridDev, mfsr_local_tone_result* res,
                                     mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && imgOut && totalWeights && statsDev && gridDev && res);
    MFSR_REQUIRE(b->haveRef && ((uintptr_t)statsDev & 7) == 0 && ((uintptr_t)gridDev & 3) == 0);
    MFSR_REQUIRE(!b->cfg.uploadRing && !stencil_on(b) && !yuv_on(b) && !b->chainOn);  // (before any work: what mfsr_burst_set_local_tone refuses)
    const Layout& L = b->L;
    mfsr_local_tone lt;
    if (ltIn)
        lt = *ltIn;
    else
        TRY(mfsr_local_tone_defaults(L.hrW, L.hrH, &lt));
    int gx = 0, gy = 0, gz = 0;
    TRY(mfsr_local_tone_grid(L.hrW, L.hrH, &lt, &gx, &gy, &gz));
    TRY(flush_pending(b, stream));
    const size_t entries = (size_t)gx * gy * gz;
    const FinishView v = finish_view(b, imgOut, totalWeights, 0, out_h(b));
    MFSR_HIP_TRY(hipMemsetAsync(statsDev, 0, sizeof(uint64_t) * 2 * entries, mfsr_s(stream)));
    TRY(mfsr_finishToneGridStats(FINISH_SOURCE(b, v), v.w, v.rows, b->cfg.weightThreshold, FINISH_PLACE(b, v),
                                 b->renderOn && b->render.useMatrix ? b->render.matrix : nullptr, &lt, statsDev, stream));
    b->toneStats.resize(2 * entries);
    MFSR_HIP_TRY(hipMemcpyAsync(b->toneStats.data(), statsDev, sizeof(uint64_t) * 2 * entries, hipMemcpyDeviceToHost, mfsr_s(stream)));
    MFSR_HIP_TRY(hipStreamSynchronize(mfsr_s(stream)));
    b->toneGrid.resize(entries);
    mfsr_local_tone_result out;
    memset(&out, 0, sizeof(out));
    TRY(mfsr_local_tone_fit(b->toneStats.data(), L.hrW, L.hrH, &lt, b->toneGrid.data(), &out.pivot, &out.status));
    out.minGain = out.maxGain = b->toneGrid[0];
    for (size_t i = 1; i < entries; i++) {
        out.minGain = b->toneGrid[i] < out.minGain ? b->toneGrid[i] : out.minGain;
        out.maxGain = b->toneGrid[i] > out.maxGain ? b->toneGrid[i] : out.maxGain;
    }
    MFSR_HIP_TRY(hipMemcpyAsync(gridDev, b->toneGrid.data(), sizeof(float) * entries, hipMemcpyHostToDevice, mfsr_s(stream)));
    MFSR_HIP_TRY(hipStreamSynchronize(mfsr_s(stream)));  // (the staging may be written again by the next call)
    TRY(mfsr_burst_set_local_tone(b, &lt, gridDev));  // (after the flush its own guard holds)
    *res = out;
    return MFSR_OK;
}

extern "C" int mfsr_burst_finish(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights,
                                 mfsr_float3* outImg, uint16_t* out16, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && imgOut && totalWeights && (outImg || out16));
    MFSR_REQUIRE(b->haveRef);
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    // The finish inside the burst launch: only the plain whole-frame uint16_t image, and only where the hold's launch (two or
    // more groups on these accumulators) is the burst's last fuse -- nothing waits behind it (with 9 frames the ninth is fused
    // after the burst launch, which then must not finish).  drain_waiting decides the rest (the entry's own refusals).
    b->finishTaken = false;
    b->finishOut16 = nullptr;
    if (finish_fuse_enabled() && c.fused && !stencil_on(b) && !b->renderOn && !b->localToneOn && !b->chainOn && !b->win.on && out16 && !outImg &&
        !c.applyGamma &&
        b->nHold >= 2 && b->pend.n == 0 && !b->heldHas && b->hold[0].imgOut == imgOut && b->hold[0].totalWeights == totalWeights)
        b->finishOut16 = out16;
    const int rcFlush = flush_pending(b, stream);
    b->finishOut16 = nullptr;
    if (rcFlush != MFSR_OK) return rcFlush;
    if (b->finishTaken) {
        b->finishTaken = false;
        return MFSR_OK;
    }
    // One launch on the accumulators (finish_rows).  A stencil takes it with cfg.fused = 0 too: it cannot run in place on the
    // chain's in/out image, and the value the fused finish holds before its gamma is bit for bit the chain's resampleFloat3 +
    // ApplyWeighting (tests/test_parity_kernels.py::test_finishFused_equals_chain), so the unfused burst's sharpened finish is
    // this launch as well: no second HR float image.  The local-tone finish (§2.25) likewise.
    if (c.fused || stencil_on(b) || b->localToneOn || b->chainOn) return finish_rows(b, imgOut, totalWeights, outImg, out16, 0, out_h(b), 0, 0, stream);
    // the unfused chain: the reference's own sequence, with the float image as its in/out buffer
    const int pitch = 12 * out_w(b);
    MFSR_REQUIRE(outImg != nullptr);
    TRY(mfsr_resampleFloat3((const mfsr_float3*)L.fallback.ptr, L.fallback.pitch, L.W, L.H, outImg, pitch, L.hrW, L.hrH,
                            0.0f, 1.0f, 0.0f, 1.0f, stream));
    TRY(mfsr_ApplyWeighting(outImg, imgOut, totalWeights, L.hrW, L.hrH, pitch, c.weightThreshold, stream));
    if (b->renderOn) {  // the pixel body on the float image in place of GammasRGB + quantize
        const int rowBytes = (int)out_row_bytes(b);
        if (yuv_on(b))
            return mfsr_renderImageYuv(outImg, pitch, outImg, pitch, out16, rowBytes,
                                       out16 ? (char*)out16 + (size_t)L.hrH * rowBytes : nullptr, rowBytes, L.hrW, L.hrH, &b->render,
                                       c.applyGamma, stream);
        return mfsr_renderImage(outImg, pitch, outImg, pitch, out16, rowBytes, L.hrW, L.hrH, &b->render, c.applyGamma, stream);
    }
    if (c.applyGamma) TRY(mfsr_GammasRGB(outImg, L.hrW, L.hrH, pitch, stream));
    if (out16) TRY(mfsr_quantize(outImg, pitch, out16, nullptr, L.hrW, L.hrH, 65535.0f, stream));
    return MFSR_OK;
}

// ---- the geometric finish: an explicit call beside mfsr_burst_finish, never a mode of it --------------------
extern "C" int mfsr_burst_finish_geometry(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights,
                                          const mfsr_geometry* geometry, mfsr_float3* outImg, int outImgRowBytes, void* out,
                                          int outRowBytes, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && imgOut && totalWeights && geometry && (outImg || out));
    MFSR_REQUIRE(b->haveRef);
    // before any work: the launch reads the whole HR frame and knows none of the other stages
    MFSR_REQUIRE(!b->win.on);
    MFSR_REQUIRE(!b->sharpenOn && !b->denoiseOn && !b->localToneOn && !b->chainOn);
    MFSR_REQUIRE(!yuv_on(b));
    TRY(mfsr_geometry_validate(geometry));
    // (finishOut16 stays null: the finish inside the burst launch is never taken here)
    b->finishTaken = false;
    b->finishOut16 = nullptr;
    TRY(flush_pending(b, stream));
    const mfsr_config& c = b->cfg;
    const FinishView v = finish_view(b, imgOut, totalWeights, 0, out_h(b));
    b->geometryFinishes++;
    return mfsr_finishGeometry(FINISH_SOURCE(b, v), b->L.hrW, b->L.hrH, outImg, outImgRowBytes, out, outRowBytes,
                               b->renderOn ? &b->render : nullptr, geometry, c.weightThreshold, c.applyGamma, 0, 0, geometry->outW,
                               geometry->outH, stream);
}

extern "C" int mfsr_burst_debug_geometry(const mfsr_burst* b, int* finishes)
{
    MFSR_REQUIRE(b && finishes);
    *finishes = b->geometryFinishes;
    return MFSR_OK;
}

// finish on the HR row stripe [row0, row0+rows): used after a reduce-scatter of
// the accumulators, where each rank normalises only its own stripe.  Pointers are
// those of the FULL images; only the stripe is read/written.
extern "C" int mfsr_burst_finish_rows(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights,
                                      mfsr_float3* outImg, uint16_t* out16, int row0, int rows, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && imgOut && totalWeights && (outImg || out16));
    MFSR_REQUIRE(b->haveRef);
    MFSR_REQUIRE(row0 >= 0 && rows > 0 && row0 + rows <= b->L.hrH);
    MFSR_REQUIRE(!b->win.on);  // (stripes of whole-frame images)
    if (yuv_on(b)) MFSR_REQUIRE((row0 & 1) == 0 && (rows & 1) == 0);  // whole 2 x 2 chroma blocks
    TRY(flush_pending(b, stream));
    int above = 0, below = 0;
    if (stencil_on(b)) stencil_reach(b, row0, rows, &above, &below);
    return finish_rows(b, imgOut, totalWeights, outImg, out16, row0, rows, above, below, stream);
}

// ---- host-frame bursts (cfg.uploadRing) --------------------------------------------------------------------------
// enqueue the upload of hostRaw into upload slot `us` on the copy stream (after the slot's last consumer) and make the
// compute stream wait for it
// A host burst captured into a graph.  The events that order one burst's copies against the burst before it (evFree, unpDone,
// evDown) hold across calls, and an event recorded outside a capture cannot be waited for inside it, nor the other way round.
// So every host entry point looks at the capture `stream` is in; when that is another one than at the last call (a capture
// began, ended, or a second one began), the events of the old one are forgotten and the copy and the download stream are
// forked off `stream` instead: they then follow everything enqueued on it so far, and inside a capture that wait is what
// makes them part of the graph.  What a graph cannot see is work of an EAGER burst still in flight on those two streams:
// mfsr_burst_host_sync before the capture, and before a replay that follows eager bursts of the same handle (mfsr.h).
// Nothing is enqueued while the capture stays the same: the eager launch sequence is untouched.
static int host_epoch(mfsr_burst* b, mfsr_stream_t stream, bool* capturing = nullptr)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo(mfsr_s(stream), &cap, &id) != hipSuccess) cap = hipStreamCaptureStatusNone;
    const unsigned long long epoch = cap == hipStreamCaptureStatusActive ? (id ? id : ~0ull) : 0;
    if (capturing) *capturing = epoch != 0;
    if (epoch == b->hostEpoch) return MFSR_OK;
    b->hostEpoch = epoch;
    for (int i = 0; i < kMaxUploadRing + 2; i++) {
        b->freeRecorded[i] = false;
        b->unpDone[i] = nullptr;
    }
    b->downRecorded = false;
    b->upPending = false;
    b->nUnp = 0;
    b->nPrefetched = b->prefetchHead = 0;
    MFSR_HIP_TRY(hipEventRecord(b->evEpoch, mfsr_s(stream)));
    MFSR_HIP_TRY(hipStreamWaitEvent(b->copyStream, b->evEpoch, 0));
    MFSR_HIP_TRY(hipStreamWaitEvent(b->downStream, b->evEpoch, 0));
    return MFSR_OK;
}

// the end of a captured host burst: the download (and any announced copy no frame consumed) joins `stream`, so that the capture
// can end; the image is in host memory when a replay of the graph has completed, and mfsr_burst_host_sync has nothing to wait for
static int join_captured(mfsr_burst* b, mfsr_stream_t stream)
{
    MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evDown, 0));
    MFSR_HIP_TRY(hipEventRecord(b->evEpoch, b->copyStream));
    MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evEpoch, 0));
    b->downRecorded = false;
    return MFSR_OK;
}

// MFSR_UPLOAD_1D=1: the round-3 form of the uploads (A/B, see upload_into)
// MFSR_HOST_BANDS: a value that begins with '0' switches the banded tail of a host burst off (mfsr_burst_add_frame_host);
// otherwise it is the number of bands, 1 .. 16 (default 8; mfsr_burst_finish_host)
struct HostBands {
    bool on;
    int count;
};
static HostBands host_bands()
{
    static const HostBands hb = [] {
        const int n = mfsr_env_int("MFSR_HOST_BANDS", 8);
        return HostBands{!mfsr_env_is0("MFSR_HOST_BANDS"), n < 1 ? 1 : (n > 16 ? 16 : n)};
    }();
    return hb;
}

static bool upload_1d()
{
    static const bool up1d = mfsr_env_is1("MFSR_UPLOAD_1D");
    return up1d;
}

static int upload_into(mfsr_burst* b, int us, uint16_t* dst, const uint16_t* hostRaw, mfsr_stream_t stream)
{
    // a host row: rowBytes of samples (or of packed bytes), hostPitch apart
    const bool isPacked = b->cfg.rawPacking != MFSR_PACK_NONE;
    const size_t rowBytes = isPacked ? (size_t)mfsr_packed_row_bytes(b->cfg.rawPacking, b->L.W) : (size_t)b->L.W * 2;
    const size_t hostPitch = b->hostRowBytes > 0 ? (size_t)b->hostRowBytes : rowBytes;
    void* to = dst;
    if (isPacked) {
        // The copy writes the slot's STAGING buffer: it waits for the unpack that read the buffer's previous frame, not for the
        // slot's consumers (the unpack waits for those, unpack_uploaded).  A slot whose unpack has not been enqueued yet is not
        // refilled before it has.
        for (int i = 0; i < b->nUnp; i++)
            if (b->unpQ[i] == us) {
                MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evUp[b->unpQ[b->nUnp - 1]], 0));
                TRY(unpack_uploaded(b, b->unpQ[b->nUnp - 1], stream));
                break;
            }
        if (b->unpDone[us]) MFSR_HIP_TRY(hipStreamWaitEvent(b->copyStream, b->unpDone[us], 0));
        b->unpDone[us] = nullptr;
        to = b->L.stage[us];
    } else if (b->freeRecorded[us]) {
        MFSR_HIP_TRY(hipStreamWaitEvent(b->copyStream, b->evFree[us], 0));
        b->freeRecorded[us] = false;
    }
    // A 2-D copy, like the download (mfsr_burst_finish_host): measured on this ROCm (tools/pcie_duplex2.py,
    // profiles/r04_pcie_duplex_mechanisms.txt), 1-D uploads queued against 2-D downloads SERIALISE -- 16 uploads + one image:
    // 8.38 ms, the sum of the two directions alone -- while 2-D uploads and 2-D downloads overlap on the full-duplex link:
    // 4.85 ms = the uploads alone.  (A 1-D download would overlap too, but it is a blit kernel whose PCIe-bound stores slow
    // the fuse launches 4-5x.)  MFSR_UPLOAD_1D=1: the round-3 form (A/B).
    // (Host rows farther apart than they are long -- mfsr_burst_set_host_row_bytes -- are the 2-D copy's source pitch: the
    // padding of a line never crosses the link.)
    if (upload_1d())
        MFSR_HIP_TRY(hipMemcpyAsync(to, hostRaw, rowBytes * b->L.H, hipMemcpyHostToDevice, b->copyStream));
    else
        MFSR_HIP_TRY(hipMemcpy2DAsync(to, rowBytes, hostRaw, hostPitch, rowBytes, (size_t)b->L.H, hipMemcpyHostToDevice, b->copyStream));
    MFSR_HIP_TRY(hipEventRecord(b->evUp[us], b->copyStream));
    if (isPacked) b->unpQ[b->nUnp++] = us;
    // the compute stream waits for it when the first kernel that reads an uploaded frame is about to be enqueued
    // (wait_uploads): ONE wait for the last upload of a group instead of one per frame -- a cross-queue wait costs the
    // compute queue ~15 us even when it is already satisfied (four in a row before a group's first kernel: 55-68 us in the
    // trace of back-to-back bursts)
    (void)stream;
    b->upPending = true;
    b->upPendingSlot = us;
    return MFSR_OK;
}

extern "C" int mfsr_burst_set_reference_host(mfsr_burst* b, const uint16_t* hostRaw, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && hostRaw);
    MFSR_REQUIRE(b->copyStream != nullptr);  // cfg.uploadRing > 0
    TRY(host_epoch(b, stream));
    TRY(flush_pending(b, stream, false));    // a frame still waiting reads the previous reference's slots
    b->nUnp = 0;                             // (packed frames the last burst announced and did not consume: never unpacked)
    static const bool adaptive = !mfsr_env_is0("MFSR_HOST_ADAPTIVE");
    b->hostBusy = false;
    if (adaptive && b->downRecorded) {
        // (an event query is not allowed while the caller's stream is being captured into a graph)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(mfsr_s(stream), &cap) == hipSuccess && cap == hipStreamCaptureStatusNone)
            b->hostBusy = hipEventQuery(b->evDown) == hipErrorNotReady;
    }
    const int i = b->refCounter++ & 1;
    const int us = b->cfg.uploadRing + i;
    // The slot's previous reference (two bursts ago) was released by that burst's mfsr_burst_finish_host -- so that this
    // upload does not wait for the tail of the burst before this one, which is still being fused and downloaded when
    // bursts come back to back.  A burst that ended another way: the slot was last read by work already enqueued on the
    // compute stream.
    if (!b->freeRecorded[us]) TRY(record_free(b, us, stream));
    b->refSlot = us;
    b->nPrefetched = b->prefetchHead = 0;
    TRY(upload_into(b, us, b->L.refRaw[i], hostRaw, stream));
    b->refHost = hostRaw;
    b->refDev = b->L.refRaw[i];
    return mfsr_burst_set_reference(b, b->refDev, stream);
}

extern "C" int mfsr_burst_add_frame_host(mfsr_burst* b, const uint16_t* hostRaw, int isReference, mfsr_float3* imgOut,
                                         mfsr_float3* totalWeights, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && hostRaw && imgOut && totalWeights);
    MFSR_REQUIRE(b->copyStream != nullptr);
    TRY(host_epoch(b, stream));
    const bool banded = host_bands().on;
    if (isReference && hostRaw == b->refHost && b->refDev)
        return add_frame_impl(b, b->refDev, 1, imgOut, totalWeights, banded, stream);
    if (b->prefetchHead < b->nPrefetched) {
        // announced by mfsr_burst_prefetch_host: the copy is already on the copy stream
        if (b->prefetched[b->prefetchHead].host == hostRaw) {
            const int ps = b->prefetched[b->prefetchHead++].slot;
            b->upPending = true;        // this frame's kernels wait for THIS frame's copy (the copy stream is in order)
            b->upPendingSlot = ps;
            return add_frame_impl(b, b->L.rawRing[ps], isReference, imgOut, totalWeights, banded, stream);
        }
        b->nPrefetched = b->prefetchHead = 0;  // another order than announced: the remaining copies are simply not used
    }
    const int us = b->upCounter++ % b->cfg.uploadRing;
    // a ring shorter than the fuse group: the slot may still hold a frame that waits for the rest of its group
    bool waiting = false, waitingHeld = false;
    for (int i = 0; i < b->pend.n; i++) waiting = waiting || b->pend.raw[i] == b->L.rawRing[us];
    for (int i = 0; b->heldHas && i < b->held.n; i++) waitingHeld = waitingHeld || b->held.raw[i] == b->L.rawRing[us];
    if (waiting)
        TRY(accumulate_pending(b, stream));
    else if (waitingHeld)
        TRY(drain_waiting(b, stream));  // only the groups before the filling one: the frames waiting in it keep their group
    TRY(upload_into(b, us, b->L.rawRing[us], hostRaw, stream));
    return add_frame_impl(b, b->L.rawRing[us], isReference, imgOut, totalWeights, banded, stream);
}

extern "C" int mfsr_burst_prefetch_host(mfsr_burst* b, const uint16_t* const* hostRaws, int nFrames, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && hostRaws && nFrames >= 0);
    MFSR_REQUIRE(b->copyStream != nullptr);
    TRY(host_epoch(b, stream));
    b->nPrefetched = b->prefetchHead = 0;
    // only at the start of a burst: no frame may be waiting in a slot the copies would overwrite
    if (b->pend.n > 0 || b->heldHas) return MFSR_OK;
    for (int k = 0; k < nFrames && b->nPrefetched < b->cfg.uploadRing; k++) {
        MFSR_REQUIRE(hostRaws[k] != nullptr);
        if (hostRaws[k] == b->refHost && b->refDev) continue;   // add_frame_host re-uses the uploaded reference
        const int us = b->upCounter++ % b->cfg.uploadRing;
        TRY(upload_into(b, us, b->L.rawRing[us], hostRaws[k], stream));
        b->prefetched[b->nPrefetched].host = hostRaws[k];
        b->prefetched[b->nPrefetched].slot = us;
        b->nPrefetched++;
    }
    b->upPending = false;   // (every consumer sets its own wait in add_frame_host)
    return MFSR_OK;
}

// finish + download in row bands.  What is still waiting to be fused (normally the burst's last group, held back by
// add_frame) is fused band by band, each band is normalised as soon as it is complete, and its u16 rows start their way to
// the host while the next band is being fused: the 6 B/px download overlaps the tail of the compute instead of following
// it.  Row-window fuse / finish are bit-identical to the whole-frame launches (the multi-GPU stripes rest on the same).
// The download is a 2-D copy: the runtime hands those to an SDMA engine, whereas hipMemcpyAsync(DeviceToHost) is carried out
// by a blit KERNEL on this ROCm (no memory-copy record in a rocprofv3 trace, a __amd_rocclr_copyBuffer dispatch instead) whose
// PCIe-bound stores slow a warp+fuse launch running beside it 4-5x (profiles/r03_e2e_timeline_blit.txt) -- as did a
// hand-written copy kernel with a 32-workgroup grid: it is the store path that clogs, not the wave slots.
// (One more stream in the context -- a second upload stream was tried -- maps two streams onto one hardware queue and costs
// 4 ms per burst: the context stays at its four streams.)
// every reader of the burst's host reference has been enqueued on `stream`: its upload slot may be refilled after them
static int release_ref_slot(mfsr_burst* b, mfsr_stream_t stream)
{
    if (b->refSlot >= 0) {
        TRY(record_free(b, b->refSlot, stream));
        b->refSlot = -1;
    }
    return MFSR_OK;
}

extern "C" int mfsr_burst_finish_host(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights,
                                      uint16_t* out16Dev, uint16_t* out16Host, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && imgOut && totalWeights && out16Dev && out16Host);
    MFSR_REQUIRE(b->downStream != nullptr);  // cfg.uploadRing > 0
    MFSR_REQUIRE(b->haveRef);
    bool capturing = false;
    TRY(host_epoch(b, stream, &capturing));
    TRY(drain_waiting(b, stream, false));  // (resident frames of a burst-hold context added before this call: before `held`)
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    // the previous image may still be on its way to the host out of out16Dev
    if (b->downRecorded) MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evDown, 0));
    int nBands = host_bands().count;
    // The bands exist for the LATENCY of one burst (its download starts after 1/8 of the tail).  A burst that was enqueued
    // while the previous one's download was still in flight (b->hostBusy: bursts back to back) gains nothing from them -- its
    // download runs under the next burst's compute anyway -- and pays 16 band-sized fuse launches + 8 finish launches for it:
    // such a burst takes MFSR_HOST_BANDS_BUSY bands (default 2).
    static const int nBandsBusy = mfsr_env_int("MFSR_HOST_BANDS_BUSY", 2);
    // (only where the image is small against the burst -- x2: 199 MB down for 265 MB up.  At x4 the download, 796 MB, is as
    // long as the burst's compute: it has to start with the first band, or the NEXT burst's finish waits for it to leave
    // out16Dev: 18.1 instead of 17.0 ms per burst with two bands)
    const int oH = out_h(b);  // the window's height when one is set
    const size_t rowBytes = out_row_bytes(b);  // rendered bytes when a render is set
    const double outBytes = (double)out_image_bytes(b), inBytes = (double)L.W * L.H * 2.0 * c.frames;
    if (b->hostBusy && nBandsBusy >= 1 && nBandsBusy < nBands && outBytes <= 1.5 * inBytes) nBands = nBandsBusy;
    bool heldGroup = b->pend.n > 0 && b->pend.imgOut == imgOut && b->pend.totalWeights == totalWeights && c.fused;
    if (b->heldHas && !(heldGroup && b->held.imgOut == imgOut && b->held.totalWeights == totalWeights)) {
        TRY(flush_pending(b, stream));  // a held group without the last one, or other accumulators: the ordinary way
        heldGroup = false;
    }
    if (!heldGroup) TRY(flush_pending(b, stream));  // (another accumulator pair, or the unfused chain: nothing to pipeline)
    if (nBands == 1 && !heldGroup) {
        TRY(mfsr_burst_finish(b, imgOut, totalWeights, nullptr, out16Dev, stream));
        MFSR_HIP_TRY(hipEventRecord(b->evFinished, mfsr_s(stream)));
        MFSR_HIP_TRY(hipStreamWaitEvent(b->downStream, b->evFinished, 0));
        // (two-plane formats: the chroma rows follow the Y rows at the same pitch, one copy of 3 oH / 2 rows)
        MFSR_HIP_TRY(hipMemcpy2DAsync(out16Host, rowBytes, out16Dev, rowBytes, rowBytes, yuv_on(b) ? (size_t)oH * 3 / 2 : (size_t)oH,
                                      hipMemcpyDeviceToHost, b->downStream));
        MFSR_HIP_TRY(hipEventRecord(b->evDown, b->downStream));
        b->downRecorded = true;
        b->nUnp = 0;  // (packed frames that were announced and not consumed are never unpacked)
        if (capturing) TRY(join_captured(b, stream));
        return release_ref_slot(b, stream);
    }
    // the groups fused band by band, in frame order: the second-to-last group where one was held, then the last
    FuseGroup gs[2];
    gs[0].n = gs[1].n = 0;
    int freshNow = 0;
    if (heldGroup) {
        TRY(align_deferred(b, b->pend, stream));
        gs[1] = b->pend;
        b->pend.n = 0;
        if (b->heldHas) {
            gs[0] = b->held;
            b->heldHas = false;
            b->held.n = 0;
        }
        TRY(join_fuse(b, stream));  // the earlier groups' launches ran on the burst's own stream
        TRY(take_fresh(b, imgOut, totalWeights, stream, &freshNow));
    }
    // bands of output rows (window rows when a window is set: y0 is a multiple of 16, so are the bands' HR rows)
    const int tileRows = (oH + 15) / 16;
    if (nBands > tileRows) nBands = tileRows;
    // A band of a stencil finish reads R rows of its neighbours (sharpened: R <= 4, denoised: R <= 3, a chain: R <= 7): band i - 1 is finished and
    // downloaded after band i has been fused (every band but the last is a multiple of 16 rows), the last one after the loop.
    // lagR0 < 0: no band waits.
    int lagI = -1, lagR0 = -1, lagR1 = -1;
    // band i = rows [r0, r1): its finish, the event that lets the download stream follow it, and its rows on their way to the host
    auto finish_band = [&](int i, int r0, int r1) -> int {
        int above = 0, below = 0;
        if (stencil_on(b)) stencil_reach(b, r0, r1 - r0, &above, &below);
        TRY(finish_rows(b, imgOut, totalWeights, nullptr, out16Dev, r0, r1 - r0, above, below, stream));
        if (!b->evBand[i]) MFSR_HIP_TRY(hipEventCreateWithFlags(&b->evBand[i], hipEventDisableTiming));
        MFSR_HIP_TRY(hipEventRecord(b->evBand[i], mfsr_s(stream)));
        MFSR_HIP_TRY(hipStreamWaitEvent(b->downStream, b->evBand[i], 0));
        MFSR_HIP_TRY(hipMemcpy2DAsync((char*)out16Host + (size_t)r0 * rowBytes, rowBytes, (const char*)out16Dev + (size_t)r0 * rowBytes,
                                      rowBytes, rowBytes, (size_t)(r1 - r0), hipMemcpyDeviceToHost, b->downStream));
        if (yuv_on(b)) {  // the band's chroma rows (r0 is a multiple of 16, r1 one or the even height)
            const size_t c0 = ((size_t)oH + (size_t)(r0 / 2)) * rowBytes;
            MFSR_HIP_TRY(hipMemcpy2DAsync((char*)out16Host + c0, rowBytes, (const char*)out16Dev + c0, rowBytes, rowBytes,
                                          (size_t)((r1 - r0) / 2), hipMemcpyDeviceToHost, b->downStream));
        }
        return MFSR_OK;
    };
    for (int i = 0; i < nBands; i++) {
        const int r0 = (int)((long long)tileRows * i / nBands) * 16;
        int r1 = (int)((long long)tileRows * (i + 1) / nBands) * 16;
        if (r1 > oH || i == nBands - 1) r1 = oH;
        if (r1 <= r0) continue;
        int fresh = freshNow;
        for (int gi = 0; gi < 2; gi++) {
            if (gs[gi].n == 0) continue;
            TRY(fuse_group(b, gs[gi], fresh, r0, r1, stream));
            fresh = 0;
        }
        if (stencil_on(b)) {
            if (lagR0 >= 0) TRY(finish_band(lagI, lagR0, lagR1));
            lagI = i;
            lagR0 = r0;
            lagR1 = r1;
            continue;
        }
        TRY(finish_band(i, r0, r1));
    }
    if (lagR0 >= 0) TRY(finish_band(lagI, lagR0, lagR1));
    for (int gi = 0; gi < 2; gi++) TRY(release_group_slots(b, gs[gi], stream));
    MFSR_HIP_TRY(hipEventRecord(b->evDown, b->downStream));
    b->downRecorded = true;
    b->nUnp = 0;  // (packed frames that were announced and not consumed are never unpacked)
    if (capturing) TRY(join_captured(b, stream));
    return release_ref_slot(b, stream);
}

extern "C" int mfsr_burst_set_host_row_bytes(mfsr_burst* b, int rowBytes)
{
    MFSR_REQUIRE(b != nullptr && b->cfg.uploadRing > 0);
    MFSR_REQUIRE(burst_idle(b));  // between bursts only
    const bool isPacked = b->cfg.rawPacking != MFSR_PACK_NONE;
    const int dense = isPacked ? mfsr_packed_row_bytes(b->cfg.rawPacking, b->L.W) : 2 * b->L.W;
    MFSR_REQUIRE(rowBytes == 0 || rowBytes >= dense);
    MFSR_REQUIRE(isPacked || (rowBytes % 2) == 0);             // uint16_t rows
    MFSR_REQUIRE(rowBytes == 0 || rowBytes == dense || !upload_1d());
    b->hostRowBytes = rowBytes;
    return MFSR_OK;
}

extern "C" int mfsr_burst_host_sync(mfsr_burst* b)
{
    MFSR_REQUIRE(b != nullptr);
    if (b->downRecorded) MFSR_HIP_TRY(hipEventSynchronize(b->evDown));
    return MFSR_OK;
}

// ---- frame-source plug-in (pull model of multi_frame_sr.cpp:18-49) ------------------------------------------------------
extern "C" int mfsr_burst_process_source(mfsr_burst* b, const mfsr_frame_source* src, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                                         mfsr_float3* outImg, uint16_t* out16, int* framesUsed, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && src && src->next_frame && imgOut && totalWeights && (outImg || out16));
    MFSR_REQUIRE(b->copyStream != nullptr);  // cfg.uploadRing >= 3: the ring slots are the buffers the source fills
    MFSR_REQUIRE(b->cfg.rawPacking == MFSR_PACK_NONE);  // the source writes uint16_t samples: no staging, no unpack
    MFSR_REQUIRE(b->cfg.reference == 0);
    if (framesUsed) *framesUsed = 0;
    if (src->reset) src->reset(src->user);
    TRY(mfsr_burst_begin(b, imgOut, totalWeights, stream));
    int n = 0;
    for (; n < b->cfg.frames; n++) {
        // frame 0 goes to a reference slot (it is read again by every later set of reference products), the others
        // through the ring; a slot is handed out once its last consumer has been enqueued
        int us;
        uint16_t* dst;
        if (n == 0) {
            const int i = b->refCounter++ & 1;
            us = b->cfg.uploadRing + i;
            dst = b->L.refRaw[i];
            TRY(flush_pending(b, stream, false));
        } else {
            us = b->upCounter++ % b->cfg.uploadRing;
            dst = b->L.rawRing[us];
            for (int i = 0; i < b->pend.n; i++)  // a ring shorter than the fuse group (see mfsr_burst_add_frame_host)
                if (b->pend.raw[i] == dst) {
                    TRY(accumulate_pending(b, stream));
                    break;
                }
        }
        if (b->freeRecorded[us]) {
            MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), b->evFree[us], 0));
            b->freeRecorded[us] = false;
        }
        const int got = src->next_frame(src->user, dst, stream);
        if (got < 0) return got;
        if (got == 0) break;  // exhausted (the reference leaves the output array empty, :42)
        if (n == 0) {
            b->refHost = nullptr;
            b->refDev = dst;
            TRY(mfsr_burst_set_reference(b, dst, stream));
        }
        TRY(mfsr_burst_add_frame(b, dst, n == 0, imgOut, totalWeights, stream));
    }
    if (framesUsed) *framesUsed = n;
    if (n == 0) return MFSR_E_INVALID;  // an empty source has no reference frame
    return mfsr_burst_finish(b, imgOut, totalWeights, outImg, out16, stream);
}

// ---- frame selection: sharpness scores (csrc/select.hip) -> reference + kept frames ----------------------
extern "C" int mfsr_select_frames(int n, const long long* sums, int candidates, float keepRatio, int* reference, int32_t* keep)
{
    MFSR_REQUIRE(n >= 1 && sums != nullptr && reference != nullptr && candidates >= 0);
    MFSR_REQUIRE(keepRatio >= 0.0f && keepRatio <= 1.0f);  // (false for NaN)
    const int m = (candidates == 0 || candidates >= n) ? n : candidates;
    int r = 0;
    for (int k = 1; k < m; k++)
        if (sums[k] > sums[r]) r = k;  // ties: the lowest index
    *reference = r;
    if (keep) {
        const double bar = (double)keepRatio * (double)sums[r];
        for (int k = 0; k < n; k++) keep[k] = (k == r || (double)sums[k] >= bar) ? 1 : 0;
    }
    return MFSR_OK;
}

// the half-resolution rectangle mfsr_burst_select_frames scores: the whole frame less a margin, or the footprint of the zoom
// window the next set_reference adopts
static void select_rect(const mfsr_burst* b, int32_t r[4])
{
    const int hw = b->L.hw, hh = b->L.hh;
    const mfsr_burst::Window& v = b->winNext;
    if (!v.on) {
        const bool margin = hw - 8 > 8 && hh - 8 > 8;
        const int m = margin ? 8 : 1;
        r[0] = m;
        r[1] = m;
        r[2] = hw - m;
        r[3] = hh - m;
        return;
    }
    const int s2 = 2 * b->cfg.scale;
    int lo[2] = {v.x0 / s2, v.y0 / s2};
    int hi[2] = {(v.x0 + v.w + s2 - 1) / s2, (v.y0 + v.h + s2 - 1) / s2};
    const int lim[2] = {hw - 1, hh - 1};
    for (int d = 0; d < 2; d++) {
        lo[d] = lo[d] < 1 ? 1 : lo[d];
        hi[d] = hi[d] > lim[d] ? lim[d] : hi[d];
        if (hi[d] <= lo[d]) {  // the footprint lies in the unscorable ring: its nearest scorable column / row
            lo[d] = lo[d] > lim[d] - 1 ? lim[d] - 1 : lo[d];
            hi[d] = lo[d] + 1;
        }
    }
    r[0] = lo[0];
    r[1] = lo[1];
    r[2] = hi[0];
    r[3] = hi[1];
}

// the result table of a raw-domain stage: `bytes` from the device to the host on this stream, complete on return
static int download(void* host, const void* dev, size_t bytes, mfsr_stream_t stream)
{
    MFSR_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, mfsr_s(stream)));
    MFSR_HIP_TRY(hipStreamSynchronize(mfsr_s(stream)));
    return MFSR_OK;
}

extern "C" int mfsr_burst_select_frames(mfsr_burst* b, int nFrames, const uint16_t* const* frames, int candidates, float keepRatio,
                                        long long* sumsDev, int* reference, int32_t* keep, long long* sums, int32_t rect[4],
                                        mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && frames && sumsDev && reference);
    MFSR_REQUIRE(nFrames >= 1 && nFrames <= b->cfg.frames);
    MFSR_REQUIRE(candidates >= 0 && keepRatio >= 0.0f && keepRatio <= 1.0f);
    const mfsr_config& c = b->cfg;
    int32_t r[4];
    select_rect(b, r);
    TRY(mfsr_frameSharpness(nFrames, frames, 2 * c.width, c.width, c.height, c.cfa, c.mono, r, sumsDev, stream));
    std::vector<long long> host((size_t)nFrames);
    TRY(download(host.data(), sumsDev, sizeof(long long) * host.size(), stream));
    std::vector<int32_t> k((size_t)nFrames);
    TRY(mfsr_select_frames(nFrames, host.data(), candidates, keepRatio, reference, k.data()));
    if (keep) memcpy(keep, k.data(), sizeof(int32_t) * (size_t)nFrames);
    if (sums) memcpy(sums, host.data(), sizeof(long long) * (size_t)nFrames);
    if (rect) memcpy(rect, r, sizeof(r));
    return MFSR_OK;
}

// ---- defective pixels: vote over the burst's frames, repair in place (csrc/defect.hip) -----------------------
extern "C" int mfsr_burst_repair_defects(mfsr_burst* b, int nFrames, uint16_t* const* frames, int threshold, int spread,
                                         int minVotes, uint8_t* mapDev, uint32_t* countsDev, uint32_t counts[2],
                                         mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && frames && mapDev);
    MFSR_REQUIRE(counts == nullptr || countsDev != nullptr);
    const mfsr_config& c = b->cfg;
    TRY(mfsr_detectDefects(nFrames, frames, 2 * c.width, c.width, c.height, c.mono, threshold, spread, minVotes, mapDev, c.width,
                           countsDev, stream));
    TRY(mfsr_repairDefects(nFrames, frames, 2 * c.width, c.width, c.height, c.mono, mapDev, c.width, stream));
    if (counts) TRY(download(counts, countsDev, 2 * sizeof(uint32_t), stream));
    return MFSR_OK;
}

// ---- exposure matching: level sums of every frame, gains against the reference, applied in place
//      (csrc/exposure.hip) ------------------------------------------------------------------------------------------------
extern "C" int mfsr_exposure_defaults(const mfsr_config* cfg, int32_t black[4], int32_t* sat, int32_t* maxValue, int32_t* deadband,
                                      int32_t* minGain, int32_t* maxGain, int32_t* perColour)
{
    MFSR_REQUIRE(cfg != nullptr);
    if (black)
        for (int q = 0; q < 4; q++) {
            const int c = cfg->mono ? 0 : cfg->cfa[q];
            MFSR_REQUIRE(c >= MFSR_RED && c <= MFSR_BLUE);
            black[q] = (int32_t)floor((double)cfg->black[c] + 0.5);
        }
    if (sat) {
        double s = floor((double)cfg->black[0] + (double)cfg->white[0]);
        for (int c = 1; c < 3; c++) {
            const double v = floor((double)cfg->black[c] + (double)cfg->white[c]);
            s = v < s ? v : s;
        }
        *sat = (int32_t)s;
    }
    if (maxValue) *maxValue = (int32_t)cfg->maxVal;
    if (deadband) *deadband = 164;
    if (minGain) *minGain = 16384;
    if (maxGain) *maxGain = 262144;
    if (perColour) *perColour = 0;
    return MFSR_OK;
}

extern "C" int mfsr_burst_match_exposure(mfsr_burst* b, int nFrames, uint16_t* const* frames, int reference, int perColour,
                                         int deadband, int minGain, int maxGain, long long* levelsDev, int32_t* gains,
                                         int32_t* status, long long* levels, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && frames && levelsDev);
    MFSR_REQUIRE(nFrames >= 1 && nFrames <= 64 && reference >= 0 && reference < nFrames);
    MFSR_REQUIRE(exposure_bounds_ok(deadband, minGain, maxGain));
    const mfsr_config& c = b->cfg;
    int32_t black[4], sat = 0, maxValue = 0, r[4];
    TRY(mfsr_exposure_defaults(&c, black, &sat, &maxValue, nullptr, nullptr, nullptr, nullptr));
    MFSR_REQUIRE(0 < sat && sat <= maxValue && maxValue <= 65535);
    select_rect(b, r);
    TRY(mfsr_frameLevels(nFrames, frames, 2 * c.width, c.width, c.height, black, sat, r, levelsDev, stream));
    std::vector<long long> host(5 * (size_t)nFrames);
    TRY(download(host.data(), levelsDev, sizeof(long long) * host.size(), stream));
    std::vector<int32_t> g(3 * (size_t)nFrames), st((size_t)nFrames);
    TRY(mfsr_exposure_gains(nFrames, host.data(), reference, c.cfa, c.mono, perColour, deadband, minGain, maxGain, g.data(), st.data()));
    TRY(mfsr_applyGains(nFrames, frames, 2 * c.width, c.width, c.height, c.cfa, c.mono, black, sat, maxValue, g.data(), st.data(), stream));
    if (gains) memcpy(gains, g.data(), sizeof(int32_t) * g.size());
    if (status) memcpy(status, st.data(), sizeof(int32_t) * st.size());
    if (levels) memcpy(levels, host.data(), sizeof(long long) * host.size());
    return MFSR_OK;
}

// ---- lens shading: a flat-field gain map applied in place (csrc/shading.hip) -------------------------------
extern "C" int mfsr_shading_defaults(const mfsr_config* cfg, int32_t black[4], int32_t* sat, int32_t* maxValue, int32_t* cell,
                                     int32_t* minQuads, int32_t* maxGain)
{
    MFSR_REQUIRE(cfg != nullptr);
    TRY(mfsr_exposure_defaults(cfg, black, sat, maxValue, nullptr, nullptr, nullptr, nullptr));
    if (cell) {
        const int m = (cfg->width < cfg->height ? cfg->width : cfg->height) / 2 - 1;
        MFSR_REQUIRE(cfg->width % 2 == 0 && cfg->height % 2 == 0 && m >= 8);  // (18 x 18 samples: two grid points each way)
        int c = 64;
        while (c > m) c >>= 1;
        *cell = c;
    }
    if (minQuads) *minQuads = 64;
    if (maxGain) *maxGain = 524288;
    return MFSR_OK;
}

extern "C" int mfsr_burst_correct_shading(mfsr_burst* b, int nFrames, uint16_t* const* frames, const int32_t* mapDev, int cell,
                                          mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && frames && mapDev);
    const mfsr_config& c = b->cfg;
    int32_t black[4], maxValue = 0, defCell = 0;
    TRY(mfsr_shading_defaults(&c, black, nullptr, &maxValue, cell > 0 ? nullptr : &defCell, nullptr, nullptr));
    return mfsr_applyShading(nFrames, frames, 2 * c.width, c.width, c.height, mapDev, cell > 0 ? cell : defCell, black, maxValue, stream);
}

// ---- noise-model calibration: block statistics of the frames on the device, the fit on the host
//      (csrc/noise.hip).  Nothing in the burst changes. -----------------------------------------------------------------
extern "C" int mfsr_noise_defaults(const mfsr_config* cfg, int32_t black[4], float white[4], int32_t* sat, int32_t* minBlocks,
                                   int32_t rect[4])
{
    MFSR_REQUIRE(cfg != nullptr);
    TRY(mfsr_exposure_defaults(cfg, black, sat, nullptr, nullptr, nullptr, nullptr, nullptr));
    if (white)
        for (int q = 0; q < 4; q++) {
            const int c = cfg->mono ? 0 : cfg->cfa[q];
            MFSR_REQUIRE(c >= MFSR_RED && c <= MFSR_BLUE);
            white[q] = cfg->white[c];
        }
    if (minBlocks) *minBlocks = 200;
    if (rect) {
        MFSR_REQUIRE(cfg->width >= 24 && cfg->height >= 24);
        rect[0] = rect[1] = 1;
        rect[2] = cfg->width / 8 - 1;
        rect[3] = cfg->height / 8 - 1;
    }
    return MFSR_OK;
}

extern "C" int mfsr_burst_calibrate_noise(mfsr_burst* b, int nFrames, const uint16_t* const* frames, void* scratchDev, float* alpha,
                                          float* beta, int32_t* status, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && frames && scratchDev && alpha && beta && status);
    MFSR_REQUIRE(nFrames >= 1 && nFrames <= 64 && ((uintptr_t)scratchDev & 7) == 0);
    const mfsr_config& c = b->cfg;
    int32_t black[4], sat = 0, minBlocks = 0, r[4];
    float white[4];
    TRY(mfsr_noise_defaults(&c, black, white, &sat, &minBlocks, r));
    uint32_t* histDev = (uint32_t*)scratchDev;
    long long* sumDev = (long long*)((char*)scratchDev + sizeof(uint32_t) * MFSR_NOISE_HIST_ENTRIES);
    long long* countDev = sumDev + MFSR_NOISE_LEVEL_ENTRIES;
    TRY(mfsr_noiseStats(nFrames, frames, 2 * c.width, c.width, c.height, black, sat, r, histDev, sumDev, countDev, stream));
    std::vector<unsigned char> host(MFSR_NOISE_SCRATCH_BYTES);
    TRY(download(host.data(), scratchDev, host.size(), stream));
    const uint32_t* hist = (const uint32_t*)host.data();
    const long long* sum = (const long long*)(host.data() + sizeof(uint32_t) * MFSR_NOISE_HIST_ENTRIES);
    double a = 0, bt = 0;
    TRY(mfsr_noise_fit(hist, sum, sum + MFSR_NOISE_LEVEL_ENTRIES, black, white, minBlocks, &a, &bt, status, nullptr));
    *alpha = (float)a;
    *beta = (float)bt;
    return MFSR_OK;
}

// ---- burst noise calibration: the frames of the burst aligned to one of them, the block statistics of their
//      differences where two frames are a whole number of quads apart (csrc/noise_temporal.hip), the fit on the host -------------
namespace {
struct TemporalScratch {
    size_t flow0, flowBytes, mask, total;  // offsets after the tables; bytes of one flow field
    int tw, th, hw, hh;
};
size_t up256(size_t v) { return (v + 255) / 256 * 256; }
bool temporal_scratch(const mfsr_config* cfg, int nFrames, TemporalScratch* s)
{
    if (cfg == nullptr || nFrames < 2 || nFrames > 64 || validate(cfg) != MFSR_OK) return false;
    s->hw = cfg->width / 2;
    s->hh = cfg->height / 2;
    s->tw = cfg->mono ? cfg->width : s->hw;
    s->th = cfg->mono ? cfg->height : s->hh;
    s->flow0 = up256(MFSR_NOISE_SCRATCH_BYTES);
    s->flowBytes = up256((size_t)8 * s->tw * s->th);
    s->mask = s->flow0 + (size_t)(nFrames - 1) * s->flowBytes;
    s->total = s->mask + up256((size_t)16 * s->hw * s->hh);
    return true;
}
}  // namespace

extern "C" size_t mfsr_noise_temporal_scratch_bytes(const mfsr_config* cfg, int nFrames)
{
    TemporalScratch s;
    return temporal_scratch(cfg, nFrames, &s) ? s.total : 0;
}

extern "C" int mfsr_burst_calibrate_noise_temporal(mfsr_burst* b, int nFrames, const uint16_t* const* frames, int reference, float tol,
                                                   int minBlocks, void* scratchDev, size_t scratchBytes, double* alpha, double* beta,
                                                   int32_t* status, int32_t* points, long long* blocks, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && frames && scratchDev && alpha && beta && status);
    MFSR_REQUIRE(nFrames >= 2 && nFrames <= 64 && reference >= 0 && reference < nFrames);
    MFSR_REQUIRE(!(tol > 0.25f) && tol == tol);  // (<= 0: the default)
    for (int k = 0; k < nFrames; k++) MFSR_REQUIRE(frames[k] != nullptr && ((uintptr_t)frames[k] & 1) == 0);
    const mfsr_config& c = b->cfg;
    TemporalScratch s;
    MFSR_REQUIRE(temporal_scratch(&c, nFrames, &s));
    MFSR_REQUIRE(((uintptr_t)scratchDev & 255) == 0 && scratchBytes >= s.total);
    if (!burst_idle(b)) {  // between bursts only
        fprintf(stderr, "mfsr: mfsr_burst_calibrate_noise_temporal with frames pending (flush or finish the burst first)\n");
        return MFSR_E_INVALID;
    }
    int32_t black[4], sat = 0, defBlocks = 0, r[4];
    float white[4];
    TRY(mfsr_noise_defaults(&c, black, white, &sat, &defBlocks, r));
    const float useTol = tol > 0.0f ? tol : 0.0625f;
    const int useBlocks = minBlocks > 0 ? minBlocks : defBlocks;

    // a new burst on this handle (what mfsr_burst_begin resets; no accumulators: nothing is fused)
    TRY(flush_pending(b, stream));
    memset(b->paths, 0, sizeof(b->paths));
    b->sharpenedFinishes = b->denoisedFinishes = b->chainedFinishes = b->geometryFinishes = 0;
    b->robustGroupLaunches = 0;
    b->fusedFinishes = 0;
    TRY(mfsr_burst_set_reference(b, frames[reference], stream));

    char* base = (char*)scratchDev;
    const uint16_t* moved[64];
    const mfsr_float2* flows[64];
    mfsr_float2* flowOut[64];
    mfsr_float4* maskOut[64];
    int m = 0;
    for (int k = 0; k < nFrames; k++) {
        if (k == reference) {
            flows[k] = nullptr;
            continue;
        }
        moved[m] = frames[k];
        flowOut[m] = (mfsr_float2*)(base + s.flow0 + (size_t)m * s.flowBytes);
        maskOut[m] = (mfsr_float4*)(base + s.mask);  // one buffer for every frame: the masks are not read
        flows[k] = flowOut[m];
        m++;
    }
    TRY(mfsr_burst_align_frames(b, m, moved, nullptr, flowOut, 8 * s.tw, maskOut, 16 * s.hw, stream));
    uint32_t* histDev = (uint32_t*)base;
    long long* sumDev = (long long*)(base + sizeof(uint32_t) * MFSR_NOISE_HIST_ENTRIES);
    long long* countDev = sumDev + MFSR_NOISE_LEVEL_ENTRIES;
    TRY(mfsr_noiseStatsTemporal(nFrames, frames, 2 * c.width, c.width, c.height, flows, 8 * s.tw, s.tw, s.th, black, sat, r, useTol,
                                histDev, sumDev, countDev, stream));
    std::vector<unsigned char> host(MFSR_NOISE_SCRATCH_BYTES);
    TRY(download(host.data(), scratchDev, host.size(), stream));
    const uint32_t* hist = (const uint32_t*)host.data();
    const long long* sum = (const long long*)(host.data() + sizeof(uint32_t) * MFSR_NOISE_HIST_ENTRIES);
    const long long* count = sum + MFSR_NOISE_LEVEL_ENTRIES;
    TRY(mfsr_noise_fit_temporal(hist, sum, count, black, white, useBlocks, alpha, beta, status, points));
    if (blocks) {
        long long n = 0;
        for (int l = 0; l < 64; l++) n += count[l];
        *blocks = n;
    }
    return MFSR_OK;
}

extern "C" int mfsr_burst_debug_views(mfsr_burst* b, mfsr_tex2d* flow, mfsr_tex2d* mask, mfsr_tex2d* kernelParam,
                                      mfsr_tex2d* tracking)
{
    MFSR_REQUIRE(b != nullptr);
    // frame-batched alignment: a frame that is still waiting for its group has no flow / mask yet (flowCur / maskCur would
    // name the previous frame's) -- the caller flushes first (mfsr_burst_flush / finish)
    if ((flow || mask) && b->pend.n > 0 && b->pend.deferred[b->pend.n - 1]) return MFSR_E_INVALID;
    if (flow) *flow = as_tex(*b->flowCur);
    if (mask) *mask = as_tex(*b->maskCur);
    if (kernelParam) *kernelParam = as_tex(b->L.kparam4);
    if (tracking) *tracking = as_tex(b->ref.pyr[0]);
    return MFSR_OK;
}

extern "C" int mfsr_burst_debug_paths(const mfsr_burst* b, int32_t* counts, int capacity, int* count)
{
    MFSR_REQUIRE(b && counts && count && capacity >= 0);
    const int n = capacity < (int)MFSR_PATH_COUNT ? capacity : (int)MFSR_PATH_COUNT;
    for (int i = 0; i < n; i++) counts[i] = b->paths[i];
    *count = (int)MFSR_PATH_COUNT;
    return MFSR_OK;
}

extern "C" int mfsr_burst_debug_frame_views(mfsr_burst* b, int framesBack, mfsr_tex2d* flow, mfsr_tex2d* mask)
{
    MFSR_REQUIRE(b != nullptr && framesBack >= 0 && framesBack < b->ring && framesBack < b->frameCounter);
    const int slot = (int)((b->frameCounter - 1 - framesBack) % b->ring);
    MFSR_REQUIRE(b->slotFlow[slot] != nullptr);
    if (flow) *flow = as_tex(*b->slotFlow[slot]);
    if (mask) *mask = as_tex(b->L.maskBuf[slot]);
    return MFSR_OK;
}

extern "C" int mfsr_burst_prealign_result(mfsr_burst* b, mfsr_prealign* hostOut, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && hostOut);
    MFSR_REQUIRE(b->cfg.preAlign && b->preCur);
    TRY(align_deferred(b, b->pend, stream));  // the last frame may still be waiting for its group: its estimate does not exist yet
    MFSR_HIP_TRY(hipMemcpyAsync(hostOut, b->preCur, sizeof(*hostOut), hipMemcpyDeviceToHost, mfsr_s(stream)));
    MFSR_HIP_TRY(hipStreamSynchronize(mfsr_s(stream)));
    return MFSR_OK;
}

// ---- frame streams: sliding window of 2R+1 frames around every frame (the reference's setTemporalAreaRadius(1),
//      finalProject/Project/multi_frame_sr.cpp:182; BASELINE configs[4]) ---------------------------------------------------
// Output t fuses frames [t-R, t+R] (clipped to the stream) with frame t as the reference: what one mfsr_burst_* burst per
// window computes.  A frame takes part in up to 2R+1 windows; its upload and its per-frame products that do not depend
// on the reference (A1 half-resolution RGB, tracking pyramid, pre-alignment search pyramid) are made once, when it
// arrives, and kept in a ring of 2R+1 entries; the burst context is handed them with every set_reference / add_frame.
namespace {
struct StreamLayout {
    size_t burstWs, accBytes, entryBytes;
    size_t offBurst, offImg, offTw, offEntries, total;
};
size_t stream_entry(const mfsr_config* c, char* base, FrameProducts* fp)
{
    const Layout L = make_layout(c, nullptr);
    Bump b{base, 0};
    const int nl = ilog2(L.maxFactor) + 1;
    FrameProducts tmp;
    memset((void*)&tmp, 0, sizeof(tmp));
    tmp.raw = (uint16_t*)b.take((size_t)L.W * L.H * 2);
    tmp.half = b.image(L.hw, L.hh, 12);
    for (int i = 0; i < nl; i++) tmp.pyr[i] = b.image(L.tw >> i, L.th >> i, 4);
    tmp.prePyr = c->preAlign ? b.take(mfsr_preAlign_pyramid_bytes(L.tw, L.th)) : nullptr;
    if (fp) *fp = tmp;
    return align_up(b.off, 256);
}
int stream_layout(const mfsr_config* c, int radius, StreamLayout* S)
{
    memset(S, 0, sizeof(*S));
    const Layout L = make_layout(c, nullptr);
    S->burstWs = L.total;
    S->accBytes = (size_t)12 * L.hrW * L.hrH;
    S->entryBytes = stream_entry(c, nullptr, nullptr);
    size_t off = 0;
    S->offBurst = off;
    off = align_up(off + S->burstWs, 256);
    S->offImg = off;
    off = align_up(off + S->accBytes, 256);
    S->offTw = off;
    off = align_up(off + S->accBytes, 256);
    S->offEntries = off;
    off += S->entryBytes * (size_t)(2 * radius + 1);
    S->total = align_up(off, 256);
    return MFSR_OK;
}
}  // namespace

struct mfsr_stream {
    mfsr_config cfg;
    int R, cap, hostFrames;
    mfsr_burst* b;
    StreamLayout S;
    mfsr_float3 *imgOut, *totalWeights;
    std::vector<FrameProducts>* fp;
    long long pushed, produced;
    // frames in host memory: uploads on a stream of their own, ordered against the windows that read the slot
    hipStream_t copyStream;
    hipEvent_t evUp, evWindow[64];   // evWindow[j % 64]: output j's work enqueued on the compute stream
    bool windowRecorded[64];
    long long lastWindow;            // index of the last output whose evWindow was recorded (-1: none)
};

extern "C" size_t mfsr_stream_workspace_bytes(const mfsr_config* cfg, int radius)
{
    if (validate(cfg) != MFSR_OK || radius < 0 || radius > 15) return 0;
    StreamLayout S;
    stream_layout(cfg, radius, &S);
    return S.total;
}

extern "C" int mfsr_stream_create(mfsr_stream** out, const mfsr_config* cfg, int radius, int framesInHostMemory, void* workspace,
                                  size_t workspaceBytes)
{
    MFSR_REQUIRE(out && workspace && radius >= 0 && radius <= 15 && ((uintptr_t)workspace & 255) == 0);
    TRY(validate(cfg));
    mfsr_stream* s = new (std::nothrow) mfsr_stream;
    MFSR_REQUIRE(s != nullptr);
    memset((void*)s, 0, sizeof(*s));
    s->cfg = *cfg;
    s->cfg.frames = 2 * radius + 1;
    s->cfg.uploadRing = 0;
    s->R = radius;
    s->cap = 2 * radius + 1;
    s->hostFrames = framesInHostMemory ? 1 : 0;
    stream_layout(&s->cfg, radius, &s->S);
    if (s->S.total > workspaceBytes) {
        fprintf(stderr, "mfsr: stream workspace too small: need %zu bytes, got %zu\n", s->S.total, workspaceBytes);
        delete s;
        return MFSR_E_WORKSPACE;
    }
    char* base = (char*)workspace;
    int rc = mfsr_burst_create(&s->b, &s->cfg, base + s->S.offBurst, s->S.burstWs);
    if (rc != MFSR_OK) {
        delete s;
        return rc;
    }
    s->imgOut = (mfsr_float3*)(base + s->S.offImg);
    s->totalWeights = (mfsr_float3*)(base + s->S.offTw);
    s->lastWindow = -1;
    s->fp = new (std::nothrow) std::vector<FrameProducts>(s->cap);
    if (!s->fp) {
        mfsr_stream_destroy(s);
        return MFSR_E_INVALID;
    }
    for (int i = 0; i < s->cap; i++) stream_entry(&s->cfg, base + s->S.offEntries + s->S.entryBytes * (size_t)i, &(*s->fp)[i]);
    if (s->hostFrames) {
        hipError_t e = hipStreamCreateWithFlags(&s->copyStream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->evUp, hipEventDisableTiming);
        for (int i = 0; i < 64 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&s->evWindow[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            mfsr_stream_destroy(s);
            return MFSR_E_NODEVICE;
        }
    }
    *out = s;
    return MFSR_OK;
}

extern "C" void mfsr_stream_destroy(mfsr_stream* s)
{
    if (!s) return;
    if (s->copyStream) (void)hipStreamSynchronize(s->copyStream);
    if (s->evUp) (void)hipEventDestroy(s->evUp);
    for (int i = 0; i < 64; i++)
        if (s->evWindow[i]) (void)hipEventDestroy(s->evWindow[i]);
    if (s->copyStream) (void)hipStreamDestroy(s->copyStream);
    mfsr_burst_destroy(s->b);
    delete s->fp;
    delete s;
}

// output j from the cached frames [lo, hi]
static int stream_window(mfsr_stream* s, long long j, long long lo, long long hi, mfsr_float3* outImg, uint16_t* out16,
                         mfsr_stream_t stream)
{
    mfsr_burst* b = s->b;
    const FrameProducts& ref = (*s->fp)[j % s->cap];
    TRY(mfsr_burst_begin(b, s->imgOut, s->totalWeights, stream));
    TRY(set_reference_impl(b, ref.raw, 0, b->L.hrH, stream, &ref));
    for (long long k = lo; k <= hi; k++) {
        const FrameProducts& f = (*s->fp)[k % s->cap];
        TRY(add_frame_impl(b, f.raw, k == j, s->imgOut, s->totalWeights, false, stream, &f));
    }
    TRY(mfsr_burst_finish(b, s->imgOut, s->totalWeights, outImg, out16, stream));
    if (s->copyStream) {
        MFSR_HIP_TRY(hipEventRecord(s->evWindow[j % 64], mfsr_s(stream)));
        s->windowRecorded[j % 64] = true;
        s->lastWindow = j;
    }
    return MFSR_OK;
}

extern "C" int mfsr_stream_push(mfsr_stream* s, const uint16_t* frame, mfsr_float3* outImg, uint16_t* out16, long long* produced,
                                mfsr_stream_t stream)
{
    MFSR_REQUIRE(s && frame && produced);
    *produced = -1;
    mfsr_burst* b = s->b;
    const Layout& L = b->L;
    const long long t = s->pushed;
    FrameProducts& f = (*s->fp)[t % s->cap];
    const size_t rawBytes = (size_t)L.W * L.H * 2;
    if (s->hostFrames) {
        // the slot held frame t - cap, last read by output t - cap + R = t - R - 1
        const long long last = t - s->R - 1;
        if (last >= 0 && s->windowRecorded[last % 64]) MFSR_HIP_TRY(hipStreamWaitEvent(s->copyStream, s->evWindow[last % 64], 0));
        // (2-D, like mfsr_burst_add_frame_host's uploads: overlaps with the 2-D downloads of a caller's results)
        MFSR_HIP_TRY(hipMemcpy2DAsync(f.raw, (size_t)L.W * 2, frame, (size_t)L.W * 2, (size_t)L.W * 2, (size_t)L.H, hipMemcpyHostToDevice,
                                      s->copyStream));
        MFSR_HIP_TRY(hipEventRecord(s->evUp, s->copyStream));
        MFSR_HIP_TRY(hipStreamWaitEvent(mfsr_s(stream), s->evUp, 0));
    } else {
        MFSR_HIP_TRY(hipMemcpyAsync(f.raw, frame, rawBytes, hipMemcpyDeviceToDevice, mfsr_s(stream)));
    }
    // per-frame products, once per frame
    TRY(prepare_frame(b, f.raw, f, stream));
    if (s->cfg.preAlign)
        TRY(mfsr_preAlignPyramid((const float*)f.pyr[0].ptr, L.tw, L.th, f.pyr[0].pitch, f.prePyr, stream));
    s->pushed = t + 1;
    if (t < s->R) return MFSR_OK;
    MFSR_REQUIRE(outImg || out16);
    const long long j = t - s->R;
    TRY(stream_window(s, j, j - s->R > 0 ? j - s->R : 0, t, outImg, out16, stream));
    s->produced = j + 1;
    *produced = j;
    return MFSR_OK;
}

extern "C" int mfsr_stream_drain(mfsr_stream* s, mfsr_float3* outImg, uint16_t* out16, long long* produced, mfsr_stream_t stream)
{
    MFSR_REQUIRE(s && produced && (outImg || out16));
    *produced = -1;
    if (s->produced >= s->pushed) return MFSR_OK;
    const long long j = s->produced;
    TRY(stream_window(s, j, j - s->R > 0 ? j - s->R : 0, s->pushed - 1, outImg, out16, stream));
    s->produced = j + 1;
    *produced = j;
    return MFSR_OK;
}

extern "C" int mfsr_stream_set_window(mfsr_stream* s, int x0, int y0, int w, int h)
{
    MFSR_REQUIRE(s != nullptr);
    MFSR_REQUIRE(s->pushed == 0);  // before the first push or after mfsr_stream_reset
    return mfsr_burst_set_window(s->b, x0, y0, w, h);  // every output's set_reference adopts it
}

extern "C" int mfsr_stream_set_render(mfsr_stream* s, const mfsr_render* render)
{
    MFSR_REQUIRE(s != nullptr);
    return mfsr_burst_set_render(s->b, render);  // every output's finish renders
}

extern "C" int mfsr_stream_set_sharpen(mfsr_stream* s, const mfsr_sharpen* sharpen)
{
    MFSR_REQUIRE(s != nullptr);
    return mfsr_burst_set_sharpen(s->b, sharpen);  // every output's finish sharpens
}

extern "C" int mfsr_stream_set_finish_chain(mfsr_stream* s, const mfsr_finish_chain* chain, const float* gridDev)
{
    MFSR_REQUIRE(s != nullptr);
    return mfsr_burst_set_finish_chain(s->b, chain, gridDev);  // every output's finish runs the chain
}

extern "C" int mfsr_stream_set_denoise(mfsr_stream* s, const mfsr_denoise* denoise)
{
    MFSR_REQUIRE(s != nullptr);
    return mfsr_burst_set_denoise(s->b, denoise);  // every output's finish denoises
}

extern "C" int mfsr_stream_reset(mfsr_stream* s)
{
    MFSR_REQUIRE(s != nullptr);
    // host-frame mode: the next push uploads into slot 0 on the copy stream, which the windows of the stream that is being
    // abandoned may still read on the compute stream: order the copy stream after the last of them (they were enqueued in
    // order), then forget their events -- index j of the new stream must not wait for output j of the old one
    if (s->copyStream && s->lastWindow >= 0 && s->windowRecorded[s->lastWindow % 64])
        MFSR_HIP_TRY(hipStreamWaitEvent(s->copyStream, s->evWindow[s->lastWindow % 64], 0));
    for (int i = 0; i < 64; i++) s->windowRecorded[i] = false;
    s->lastWindow = -1;
    s->pushed = s->produced = 0;
    return MFSR_OK;
}

// ---- whole burst with the joint shift minimiser (stage C of SURVEY.md section 3.3; ShiftMinimizerKernels.cu) ----------------
// Besides every (reference, k) pair the tile tracker also measures every neighbouring pair (k, k+1); per tile the
// N-1 frame-to-frame shifts are the least-squares solution of those m measurements (design matrix: a contiguous run of
// ones per pair, ShiftMinimizerKernels.cu:137), pairs whose residual exceeds 1 px^2 are dropped one at a time and the
// system is solved again (checkForOutliers :81-139), and the reference->k tile shifts are the signed prefix sums
// (getOptimalShifts :179-218).  Those shifts then replace the tracker's in the per-frame chain D (flow field + LK) -> F -> G.
// One fixed launch sequence, no host round trip: the solve/reject loop runs per tile inside mfsr_minimizeShiftsFused.
namespace {
struct JointLayout {
    int N, m, n1, tiles, tcx, tcy;
    size_t entryBytes;
    size_t offEntries, offPairShifts, offRefSq, offMatrix, offMeasured, offOneToOne, offOptimT, offStatus, offInfo, offPtrs, offPitches,
        offOptimal, total;
    int pairPitch;
    size_t pairBytes, refSqBytes;
};
int joint_pairs(int N, int ref, int (*pairs)[2])
{
    int m = 0;
    for (int k = 0; k + 1 < N; k++) {  // neighbours first
        if (pairs) {
            pairs[m][0] = k;
            pairs[m][1] = k + 1;
        }
        m++;
    }
    for (int k = 0; k < N; k++) {  // then the reference against every frame that is not its neighbour
        const int a = k < ref ? k : ref, bb = k < ref ? ref : k;
        if (bb - a < 2) continue;
        if (pairs) {
            pairs[m][0] = a;
            pairs[m][1] = bb;
        }
        m++;
    }
    return m;
}
void joint_layout(const mfsr_config* c, JointLayout* J)
{
    memset(J, 0, sizeof(*J));
    const Layout L = make_layout(c, nullptr);
    const int last = c->levels - 1;
    J->N = c->frames;
    J->n1 = c->frames - 1;
    J->m = joint_pairs(c->frames, c->reference, nullptr);
    J->tcx = L.tcx[last];
    J->tcy = L.tcy[last];
    J->tiles = J->tcx * J->tcy;
    J->entryBytes = stream_entry(c, nullptr, nullptr);
    J->pairPitch = (int)align_up((size_t)J->tcx * 8, 64);
    J->pairBytes = align_up((size_t)J->pairPitch * J->tcy, 256);
    size_t refSq = 0;
    for (int l = 0; l < c->levels; l++) refSq += align_up((size_t)L.tcx[l] * L.tcy[l] * 4, 256);
    J->refSqBytes = refSq;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        off = align_up(off, 256);
        const size_t o = off;
        off += bytes;
        return o;
    };
    J->offEntries = take(J->entryBytes * (size_t)J->N);
    J->offPairShifts = take(J->pairBytes * (size_t)J->m);
    J->offRefSq = take(J->refSqBytes * (size_t)J->N);
    J->offMatrix = take(sizeof(float) * (size_t)J->tiles * J->n1 * J->m);
    J->offMeasured = take(8 * (size_t)J->tiles * J->m);
    J->offOneToOne = take(8 * (size_t)J->tiles * J->n1);
    J->offOptimT = take(sizeof(float) * 2 * (size_t)J->tiles * J->m);
    J->offStatus = take(sizeof(int) * (size_t)J->tiles);
    J->offInfo = take(sizeof(int) * (size_t)J->tiles);
    J->offPtrs = take(sizeof(void*) * (size_t)J->m);
    J->offPitches = take(sizeof(int) * (size_t)J->m);
    J->offOptimal = take(J->pairBytes);
    J->total = align_up(off, 256);
}
}  // namespace

extern "C" size_t mfsr_burst_joint_workspace_bytes(const mfsr_config* cfg)
{
    if (validate(cfg) != MFSR_OK || cfg->frames < 2 || cfg->frames - 1 > 63) return 0;
    JointLayout J;
    joint_layout(cfg, &J);
    return J.total;
}

extern "C" int mfsr_burst_process_joint(mfsr_burst* b, const uint16_t* const* frames, void* jointWorkspace, size_t jointBytes,
                                        mfsr_float3* imgOut, mfsr_float3* totalWeights, mfsr_stream_t stream)
{
    MFSR_REQUIRE(b && frames && jointWorkspace && imgOut && totalWeights && ((uintptr_t)jointWorkspace & 255) == 0);
    const mfsr_config& c = b->cfg;
    const Layout& L = b->L;
    MFSR_REQUIRE(c.frames >= 2 && c.frames - 1 <= 63);
    if (c.preAlign || !c.fused) {
        fprintf(stderr, "mfsr: the joint mode needs cfg.fused = 1 and cfg.preAlign = 0 (the minimiser sums tracked shifts only)\n");
        return MFSR_E_UNSUPPORTED;
    }
    JointLayout J;
    joint_layout(&c, &J);
    if (J.total > jointBytes) {
        fprintf(stderr, "mfsr: joint workspace too small: need %zu bytes, got %zu\n", J.total, jointBytes);
        return MFSR_E_WORKSPACE;
    }
    for (int k = 0; k < c.frames; k++) MFSR_REQUIRE(frames[k] != nullptr);
    char* base = (char*)jointWorkspace;
    const int N = c.frames, last = c.levels - 1;
    std::vector<FrameProducts> fp(N);
    TRY(flush_pending(b, stream, false));
    // per-frame products of every frame (each serves as reference and as moved frame of some pair)
    for (int k = 0; k < N; k++) {
        stream_entry(&c, base + J.offEntries + J.entryBytes * (size_t)k, &fp[k]);
        fp[k].raw = const_cast<uint16_t*>(frames[k]);  // read only
        TRY(prepare_frame(b, frames[k], fp[k], stream));
    }
    // sum(ref^2) tables of every frame that is the first of a pair
    int pairs[2 * 64][2];
    const int m = joint_pairs(N, c.reference, pairs);
    auto refsq_of = [&](int k, int l) {
        size_t o = 0;
        for (int i = 0; i < l; i++) o += align_up((size_t)L.tcx[i] * L.tcy[i] * 4, 256);
        return (float*)(base + J.offRefSq + J.refSqBytes * (size_t)k + o);
    };
    std::vector<char> haveSq(N, 0);
    const AlignScratch& work = L.work[0];  // (every pair is tracked in the burst's first scratch, one after the other)
    // B: every pair through the coarse -> fine tracker
    const float2* hostPtrs[2 * 64];
    int hostPitches[2 * 64];
    for (int p = 0; p < m; p++) {
        const int a = pairs[p][0], bb = pairs[p][1];
        float* refSq[kMaxLevels] = {};
        for (int l = 0; l < c.levels; l++) {
            refSq[l] = refsq_of(a, l);
            if (!haveSq[a]) {
                const Img& ref = fp[a].pyr[ilog2(c.levelFactor[l])];
                TRY(mfsr_tileSquaredSums((const float*)ref.ptr, refSq[l], ref.w, ref.h, ref.pitch, c.maxShift[l], c.tileSize[l],
                                         L.tcx[l], L.tcy[l], stream));
            }
        }
        haveSq[a] = 1;
        TRY(track_tiles(b, fp[a], refSq, fp[bb], work, nullptr, stream));
        char* dst = base + J.offPairShifts + J.pairBytes * (size_t)p;
        MFSR_HIP_TRY(hipMemcpy2DAsync(dst, J.pairPitch, work.shifts[last].ptr, work.shifts[last].pitch, (size_t)J.tcx * 8, J.tcy,
                                      hipMemcpyDeviceToDevice, mfsr_s(stream)));
        hostPtrs[p] = (const float2*)dst;
        hostPitches[p] = J.pairPitch;
    }
    // C: [tile][m] measurements, design matrix, per-tile solve / reject loop, prefix sums
    b->jointHost.assign((size_t)J.n1 * m + 2 * (size_t)m * sizeof(void*) / sizeof(float) + 2 * m + 8, 0.0f);
    float* hA = b->jointHost.data();  // column-major m x n1 (ShiftMinimizerKernels.cu:137): row p has ones in columns a..b-1
    for (int p = 0; p < m; p++)
        for (int col = pairs[p][0]; col < pairs[p][1]; col++) hA[p + (size_t)col * m] = 1.0f;
    char* hTail = (char*)(hA + (size_t)J.n1 * m);
    hTail = (char*)(((uintptr_t)hTail + 15) & ~(uintptr_t)15);
    memcpy(hTail, hostPtrs, sizeof(void*) * m);
    memcpy(hTail + sizeof(void*) * m, hostPitches, sizeof(int) * m);
    float* dA = (float*)(base + J.offMatrix);
    MFSR_HIP_TRY(hipMemcpyAsync(dA, hA, sizeof(float) * (size_t)J.n1 * m, hipMemcpyHostToDevice, mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemcpyAsync(base + J.offPtrs, hTail, sizeof(void*) * m, hipMemcpyHostToDevice, mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemcpyAsync(base + J.offPitches, hTail + sizeof(void*) * m, sizeof(int) * m, hipMemcpyHostToDevice, mfsr_s(stream)));
    TRY(mfsr_copyShiftMatrix(dA, J.tiles, N, m, stream));
    mfsr_float2* measured = (mfsr_float2*)(base + J.offMeasured);
    TRY(mfsr_concatenateShifts((const mfsr_float2* const*)(base + J.offPtrs), (int*)(base + J.offPitches), measured, m, J.tcx, J.tcy,
                               stream));
    mfsr_float2* oneToOne = (mfsr_float2*)(base + J.offOneToOne);
    TRY(mfsr_minimizeShiftsFused(dA, measured, oneToOne, (float*)(base + J.offOptimT), (int*)(base + J.offStatus),
                                 (int*)(base + J.offInfo), J.tiles, N, m, stream));
    // D, F, G per frame with the minimiser's tile shifts.  From set_reference on the burst's reference products are
    // fp[c.reference], in the caller's joint workspace: whatever the outcome, the next frame needs a new set_reference
    // (set_reference also takes the reference's tile sums again, into the burst's own table: same values, never read here)
    Img optimal;
    optimal.ptr = base + J.offOptimal;
    optimal.pitch = J.pairPitch;
    optimal.w = J.tcx;
    optimal.h = J.tcy;
    auto fuse = [&]() -> int {
        TRY(mfsr_burst_begin(b, imgOut, totalWeights, stream));
        TRY(set_reference_impl(b, frames[c.reference], 0, L.hrH, stream, &fp[c.reference]));
        for (int k = 0; k < N; k++) {
            const bool isRef = k == c.reference;
            if (!isRef)
                TRY(mfsr_getOptimalShifts((mfsr_float2*)optimal.ptr, oneToOne, N, J.tcx, J.tcy, optimal.pitch, c.reference, k, stream));
            TRY(add_frame_impl(b, frames[k], isRef, imgOut, totalWeights, false, stream, isRef ? nullptr : &fp[k],
                               isRef ? nullptr : &optimal));
        }
        return mfsr_burst_flush(b, stream);
    };
    const int rc = fuse();
    b->refStale = true;
    return rc;
}

// ---- C: joint shift minimiser driver (solve -> checkForOutliers until every tile
//      reports -1).  status/inversionInfo are device arrays of tileCount ints; the
//      loop is bounded by shiftCount rounds and polls the device once per round. ----
extern "C" int mfsr_minimizeShifts(float* shiftMatrix, mfsr_float2* measuredShifts, mfsr_float2* shiftsOneToOne,
                                   float* optimShiftsT, int* status, int* inversionInfo, int tileCount, int imageCount,
                                   int shiftCount, int* roundsOut, mfsr_stream_t stream)
{
    MFSR_REQUIRE(shiftMatrix && measuredShifts && shiftsOneToOne && optimShiftsT && status && inversionInfo);
    MFSR_REQUIRE(tileCount > 0 && imageCount > 1 && shiftCount > 0);
    MFSR_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int) * (size_t)tileCount, mfsr_s(stream)));
    int* hstatus = new (std::nothrow) int[tileCount];
    MFSR_REQUIRE(hstatus != nullptr);
    int rounds = 0, rc = MFSR_OK;
    for (; rounds < shiftCount + 1; rounds++) {
        rc = mfsr_solveShiftsBatched(shiftMatrix, measuredShifts, shiftsOneToOne, optimShiftsT, inversionInfo, tileCount,
                                     imageCount, shiftCount, stream);
        if (rc) break;
        rc = mfsr_checkForOutliers(measuredShifts, optimShiftsT, shiftMatrix, status, inversionInfo, tileCount, imageCount,
                                   shiftCount, stream);
        if (rc) break;
        hipError_t e = hipMemcpyAsync(hstatus, status, sizeof(int) * (size_t)tileCount, hipMemcpyDeviceToHost, mfsr_s(stream));
        if (e == hipSuccess) e = hipStreamSynchronize(mfsr_s(stream));
        if (e != hipSuccess) {
            rc = (int)e;
            break;
        }
        bool done = true;
        for (int i = 0; i < tileCount; i++)
            if (hstatus[i] >= 0) {
                done = false;
                break;
            }
        if (done) {
            rounds++;
            break;
        }
    }
    delete[] hstatus;
    if (roundsOut) *roundsOut = rounds;
    return rc;
}
