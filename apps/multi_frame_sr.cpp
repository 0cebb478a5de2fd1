// multi_frame_sr -- drop-in for the reference CLI
//   finalProject/Project/multi_frame_sr.cpp:122-210
//   ./multi_frame_sr optFlowName inputName iterations
// Same argv, same dataset table (city / car / iso), same outputs
// (<input>_<flow>_sr_result.png and the sharpenImg2'ed <input>_<flow>_sr2_result.png)
// and the same "sec" / "FPS" prints, but the burst goes through the MI355X hot
// path (C-ABI of include/mfsr.h) instead of OpenCV's BTVL1.
//
// Differences that are inherent to the swap (documented, not hidden):
//   * optFlowName (farneback|tvl1|brox|pyrlk) selected an OpenCV optical-flow
//     back end; here every name maps to the built-in tile tracker + Lucas-Kanade
//     refinement, `iterations` sets the number of LK iterations.
//   * frames are 8-bit RGB files; they are re-mosaicked to an RGGB 12-bit raw
//     frame (value*16) because the hot path consumes raw frames.
//   * the reference replays the burst num_times=10 times through a temporal
//     window and times the second half; here every replay is one whole burst and
//     the second half of the replays is timed (same warm-up/timed split, :146-149,:188-206).
//   * image I/O (apps/image_io.hpp): PNG (zlib), binary PGM/PPM and baseline JPEG (the "car" burst) in, PNG out.
//   * MFSR_GPUS=n in the environment (argv stays the reference's) shards the burst over n GPUs from this ONE process:
//     mfsr_dist_group (include/mfsr_dist.h) -- one worker thread per GPU inside the library, alignment sharded over
//     frames, fuse over HR row stripes, peer copies over xGMI; the u16 result is bit-identical to the 1-GPU burst.
//     MFSR_VIRTUAL_RANKS=1 puts all n ranks on device 0 (test rehearsal on a one-GPU box).
//   * MFSR_DEFECTS=1 (with MFSR_DEFECT_THRESHOLD / MFSR_DEFECT_SPREAD / MFSR_DEFECT_VOTES) repairs hot / dead pixels found
//     by a vote over the burst's frames before anything else; one GPU only.
//   * MFSR_EXPOSURE=1 (=rgb: one gain per colour) matches every frame's exposure to the reference's after the repair and the
//     selection and prints one line per frame (Q16 gains, status) to stderr; one GPU only.
//   * MFSR_NOISE=auto measures the noise model of the robustness stage (cfg.alpha, cfg.beta) on the input frames, after the
//     steps above and before the burst is created, and prints `noise: alpha A beta B status S` to
//     stderr (a status other than 0 keeps the defaults); MFSR_NOISE=alpha,beta sets the two values; one GPU only.
//     MFSR_NOISE=burst measures it on the burst itself instead: the kept frames are aligned to the reference by a throw-away
//     burst handle and the statistics are taken on the differences of frames a whole number of quads apart, where scene
//     texture cancels; it prints `noise: alpha A beta B status S points P blocks N`.
//   * MFSR_MASK_ERODE=1|2 erodes every moved frame's certainty mask by that radius before the merge (ghost suppression,
//     DESIGN.md section 2.16; 2 = the 5x5 minimum); works with MFSR_GPUS > 1.
//   * MFSR_SHARPEN="amount[,sigma[,radius[,threshold]]]" sharpens _sr_result inside the finish (an unsharp mask on the linear
//     value), with or without MFSR_CCM; one GPU only.
//   * MFSR_DENOISE="strength[,radius[,gain]]" denoises _sr_result inside the finish (a range filter whose tolerance follows the
//     accumulated weight), with or without MFSR_CCM; not with MFSR_SHARPEN; one GPU only.
//   * MFSR_LOCAL_TONE="shadows[,highlights[,cell[,bins]]]" lifts the shadows of _sr_result locally inside the finish (a bilateral
//     grid of gains measured on the merged image), with or without MFSR_CCM and MFSR_AUTO; it prints
//     `local tone: cell C bins N pivot P gains LO .. HI` on stderr; not with MFSR_SHARPEN or MFSR_DENOISE; one GPU only.
//   * MFSR_LENS="k1[,k2[,k3[,lateralR,lateralB]]]" and / or MFSR_OUT_SIZE="WxH" write _sr_result through the geometric finish
//     (mfsr_burst_finish_geometry): resampled to W x H (default: the x2 size) with the radial
//     distortion k1..k3 and the lateral magnifications of red and blue corrected (default: none), Catmull-Rom, with or without
//     MFSR_CCM and MFSR_AUTO; _sr2_result stays the sharpenImg2 pass of the x2 image; not with MFSR_SHARPEN, MFSR_DENOISE or
//     MFSR_LOCAL_TONE; one GPU only.
//   * MFSR_AUTO=wb|tone|wb,tone measures white-balance gains and / or a tone table on the merged image and renders _sr_result
//     with them, with or without MFSR_CCM and MFSR_SHARPEN; it prints `auto: gains R G B ... black K
//     white W gamma G ...` to stderr; one GPU only.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mfsr.h"
#include "../include/mfsr_dist.h"
#include "image_io.hpp"

#define HIP_OK(x)                                                                   \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));          \
            return 1;                                                               \
        }                                                                           \
    } while (0)
#define MFSR_OK_OR_DIE(x)                                                           \
    do {                                                                            \
        int rc_ = (x);                                                              \
        if (rc_ != MFSR_OK) {                                                       \
            fprintf(stderr, "%s failed: %s\n", #x, mfsr_error_string(rc_));         \
            return 1;                                                               \
        }                                                                           \
    } while (0)

int main(int argc, char** argv)
{
    std::string optFlowName, inputName;
    int iterations = 10;
    if (argc == 1) {  // multi_frame_sr.cpp:126-128
        optFlowName = "farneback";
        inputName = "city";
    } else if (argc == 4) {
        optFlowName = argv[1];
        inputName = argv[2];
        iterations = atoi(argv[3]);
        if (iterations < 1) iterations = 1;
    } else {  // :138-142
        printf("./multi_frame_sr optFlowName inputName iterations\n");
        printf("\toptFlowName: farneback, tvl1, brox, pyrlk\n");
        printf("\tinputName: city, car, iso\n");
        printf("\titerations: integer, 1, 10, etc.\n");
        return -1;
    }
    if (optFlowName != "farneback" && optFlowName != "tvl1" && optFlowName != "brox" && optFlowName != "pyrlk") {
        fprintf(stderr, "Incorrect Optical Flow algorithm - %s\n", optFlowName.c_str());  // :84
        return -1;
    }
    const int scale = 2, num_times = 10, real_times = 5;  // :146-149
    int num_images = 5;
    std::string filenameFormat;
    if (inputName == "city") {
        num_images = 5;
        filenameFormat = "img_%06d.png";
    } else if (inputName == "car") {
        num_images = 4;
        filenameFormat = "car/%d.jpg";
    } else if (inputName == "iso") {
        num_images = 4;
        filenameFormat = "iso/%06d.png";
    } else {
        printf("wrong input\n");
        return -1;
    }

    // load the burst.  The reference indexes its frames i%num_images+1 (multi_frame_sr.cpp:171) while the frames bundled
    // with it are numbered from 0 (test_opencv/img_00000[0-4].png): use 1-based names when the last 1-based file exists,
    // 0-based names otherwise.
    std::vector<Image8> imgs(num_images);
    char buf[BUFSIZ];
    int firstIndex = 1;
    {
        snprintf(buf, sizeof(buf), filenameFormat.c_str(), num_images);
        FILE* probe = fopen(buf, "rb");
        if (probe)
            fclose(probe);
        else
            firstIndex = 0;
    }
    for (int i = 0; i < num_images; i++) {
        snprintf(buf, sizeof(buf), filenameFormat.c_str(), i + firstIndex);
        if (!read_image(buf, imgs[i])) {
            fprintf(stderr, "cannot read frame %d of '%s' (%s): PNG, binary PNM, baseline JPEG or uncompressed TIFF expected\n", i, inputName.c_str(), buf);
            return 1;
        }
        printf("%s, [%d x %d]\n", buf, imgs[i].w, imgs[i].h);
        if (imgs[i].w != imgs[0].w || imgs[i].h != imgs[0].h) {
            fprintf(stderr, "frame sizes differ\n");
            return 1;
        }
    }
    const int W = imgs[0].w & ~3, H = imgs[0].h & ~3;  // the pipeline needs multiples of 4
    if (mfsr_device_count() <= 0) {
        fprintf(stderr, "no HIP device: this build has no CPU fallback\n");
        return 1;
    }

    // re-mosaic 8-bit RGB (or gray) to a 12-bit RGGB raw frame; 16-bit sources (TIFF) keep their upper 12 bits, and a
    // single-channel 16-bit frame IS the raw frame (an RGGB mosaic as the sensor delivers it)
    bool wide = !imgs[0].px16.empty();
    for (int k = 0; k < num_images; k++)
        if (wide != !imgs[k].px16.empty() || imgs[k].ch != imgs[0].ch) {
            fprintf(stderr, "frames differ in sample depth or channel count\n");
            return 1;
        }
    std::vector<std::vector<uint16_t>> raws(num_images, std::vector<uint16_t>((size_t)W * H));
    for (int k = 0; k < num_images; k++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t o = ((size_t)y * imgs[k].w + x) * imgs[k].ch;
                const int c = imgs[k].ch >= 3 ? (y & 1) + (x & 1) : 0;  // RGGB
                raws[k][(size_t)y * W + x] = wide ? (uint16_t)(imgs[k].px16[o + c] >> 4) : (uint16_t)(imgs[k].px[o + c] * 16);
            }

    mfsr_config cfg;
    MFSR_OK_OR_DIE(mfsr_config_default(&cfg, W, H, num_images, scale, 0));
    cfg.lkIterations = iterations;
    cfg.preAlign = 1;  // hand-held bursts: base shift + rotation per frame before the tile tracker (the bundled city frames
                       // are rotated by up to 15 degrees, test_opencv/main.cpp:1896)
    const float whiteLevel = wide ? 4095.0f : 4080.0f;  // 255 * 16, or the 12 bits kept of a 16-bit sample
    for (int c = 0; c < 3; c++) {
        cfg.black[c] = 0.0f;
        cfg.white[c] = whiteLevel;
    }
    cfg.maxVal = whiteLevel;
    const int hrW = W * scale, hrH = H * scale;
    const int start_i = num_times - real_times;
    std::chrono::steady_clock::time_point t0;
    std::vector<uint8_t> h8((size_t)hrW * hrH * 3), h8s(h8.size());
    uint8_t *d8 = nullptr, *d8s = nullptr;

    int gpus = 1;
    if (const char* e = getenv("MFSR_GPUS")) gpus = atoi(e);
    int selectCandidates = -1;  // MFSR_SELECT: < 0 = off (frame 0 is the reference, every frame is fused)
    float keepRatio = 0.0f;
    if (const char* e = getenv("MFSR_SELECT")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end != '\0' || v < 0 || v > 1000000) {
            fprintf(stderr, "MFSR_SELECT=%s: a number of candidate frames (0 = all) expected\n", e);
            return 1;
        }
        selectCandidates = (int)v;
        if (const char* r = getenv("MFSR_KEEP_RATIO")) {
            keepRatio = strtof(r, &end);
            if (end == r || *end != '\0') {
                fprintf(stderr, "MFSR_KEEP_RATIO=%s: a number in [0, 1] expected\n", r);
                return 1;
            }
        }
    }
    // MFSR_DEFECTS=1: find the burst's hot / dead pixels by a vote over its frames and repair them in the raw frames first
    bool defects = false;
    int defThreshold = (int)whiteLevel / 64, defSpread = 2, defVotes = num_images / 2 + 1;
    if (defVotes < (3 * num_images + 3) / 4) defVotes = (3 * num_images + 3) / 4;
    if (defThreshold < 1) defThreshold = 1;
    if (const char* e = getenv("MFSR_DEFECTS")) {
        if (strcmp(e, "0") != 0 && strcmp(e, "1") != 0) {
            fprintf(stderr, "MFSR_DEFECTS=%s: 0 or 1 expected\n", e);
            return 1;
        }
        defects = e[0] == '1';
        const struct {
            const char* name;
            int* value;
            long lo, hi;
            const char* what;
        } vars[3] = {{"MFSR_DEFECT_THRESHOLD", &defThreshold, 0, 65535, "a number in [0, 65535]"},
                     {"MFSR_DEFECT_SPREAD", &defSpread, 0, 16, "a number in [0, 16]"},
                     {"MFSR_DEFECT_VOTES", &defVotes, num_images / 2 + 1, num_images, "more than half of the frames, at most all"}};
        for (const auto& v : vars)
            if (const char* r = getenv(v.name)) {
                char* end = nullptr;
                const long x = strtol(r, &end, 10);
                if (end == r || *end != '\0' || x < v.lo || x > v.hi) {
                    fprintf(stderr, "%s=%s: %s expected\n", v.name, r, v.what);
                    return 1;
                }
                *v.value = (int)x;
            }
    }
    // MFSR_EXPOSURE=1: match every frame's exposure to the reference's (one gain per frame; =rgb: one per frame and colour)
    int exposure = 0;  // 0 off, 1 common gain, 2 per colour
    if (const char* e = getenv("MFSR_EXPOSURE")) {
        if (strcmp(e, "0") != 0 && strcmp(e, "1") != 0 && strcmp(e, "rgb") != 0) {
            fprintf(stderr, "MFSR_EXPOSURE=%s: 0, 1 or rgb expected\n", e);
            return 1;
        }
        exposure = e[0] == 'r' ? 2 : e[0] == '1' ? 1 : 0;
    }
    // MFSR_SHADING=<16-bit binary PGM>: a lens-shading gain map, gw x 4*gh pixels (the four quad positions' planes stacked),
    // Q12 (gain = value / 4096, never below 1.0); MFSR_SHADING_CELL=<cell in quads> (default: mfsr_shading_defaults)
    std::vector<int32_t> shadingMap;
    int shadingCell = 0, shadingGw = 0, shadingGh = 0;
    if (const char* e = getenv("MFSR_SHADING")) {
        int32_t cell = 0;
        if (const char* r = getenv("MFSR_SHADING_CELL")) {
            char* end = nullptr;
            const long x = strtol(r, &end, 10);
            if (end == r || *end != '\0' || x < 8 || x > 256 || (x & (x - 1)) != 0) {
                fprintf(stderr, "MFSR_SHADING_CELL=%s: a power of two in [8, 256] expected\n", r);
                return 1;
            }
            cell = (int32_t)x;
        } else if (mfsr_shading_defaults(&cfg, nullptr, nullptr, nullptr, &cell, nullptr, nullptr) != MFSR_OK) {
            fprintf(stderr, "MFSR_SHADING: frames of at least 18 x 18 samples expected\n");
            return 1;
        }
        shadingCell = cell;
        shadingGw = (W / 2 - 2 + cell) / cell + 1;
        shadingGh = (H / 2 - 2 + cell) / cell + 1;
        int mw = 0, mh = 0;
        std::vector<uint16_t> px;
        if (!read_pgm16(e, mw, mh, px)) {
            fprintf(stderr, "MFSR_SHADING=%s: cannot read a binary PGM with 16-bit samples (maxval 65535)\n", e);
            return 1;
        }
        if (mw != shadingGw || mh != 4 * shadingGh) {
            fprintf(stderr, "MFSR_SHADING=%s: the map is %d x %d, but cell %d on %d x %d frames needs %d x %d (gw x 4*gh)\n", e, mw, mh,
                    cell, W, H, shadingGw, 4 * shadingGh);
            return 1;
        }
        shadingMap.resize(px.size());
        for (size_t i = 0; i < px.size(); i++) {
            if (px[i] < 4096) {
                fprintf(stderr, "MFSR_SHADING=%s: value %d at map pixel %zu is below 4096 (Q12: a gain below 1.0)\n", e, (int)px[i], i);
                return 1;
            }
            shadingMap[i] = (int32_t)px[i] * 16;
        }
    }
    // MFSR_NOISE=auto: calibrate cfg.alpha / cfg.beta on the input frames; MFSR_NOISE=burst: on the differences of the aligned
    // frames of the burst; MFSR_NOISE=alpha,beta: set them
    int noiseMode = 0;  // 0 off, 1 auto, 2 given, 3 burst
    if (const char* e = getenv("MFSR_NOISE")) {
        if (strcmp(e, "auto") == 0)
            noiseMode = 1;
        else if (strcmp(e, "burst") == 0)
            noiseMode = 3;
        else {
            char *end = nullptr, *end2 = nullptr;
            const float a = strtof(e, &end);
            const float bt = (end != e && *end == ',') ? strtof(end + 1, &end2) : 0.0f;
            if (end == e || *end != ',' || end2 == end + 1 || *end2 != '\0' || !(a > 0.0f) || !(bt >= 0.0f) || !(a < 1.0f) || !(bt < 1.0f)) {
                fprintf(stderr, "MFSR_NOISE=%s: auto, burst, or alpha,beta (0 < alpha < 1, 0 <= beta < 1) expected\n", e);
                return 1;
            }
            cfg.alpha = a;
            cfg.beta = bt;
            noiseMode = 2;
        }
    }
    // MFSR_MASK_ERODE=1|2: erode every moved frame's certainty mask by that radius before the merge (cfg.maskErode); it is
    // part of the alignment stage, so a burst sharded over several GPUs takes it as well
    if (const char* e = getenv("MFSR_MASK_ERODE")) {
        if (strcmp(e, "0") != 0 && strcmp(e, "1") != 0 && strcmp(e, "2") != 0) {
            fprintf(stderr, "MFSR_MASK_ERODE=%s: 0, 1 or 2 expected\n", e);
            return 1;
        }
        cfg.maskErode = e[0] - '0';
    }
    // MFSR_CCM="m00,m01,...,m22": a 3x3 colour matrix (row-major, display RGB = matrix * camera RGB); the 8-bit image then comes
    // out of the rendered finish (mfsr_burst_set_render, MFSR_OUT_RGB8) instead of the float image + mfsr_quantize
    bool ccm = false;
    mfsr_render render;
    memset(&render, 0, sizeof(render));
    if (const char* e = getenv("MFSR_CCM")) {
        const char* p = e;
        bool ok = true;
        for (int i = 0; i < 9 && ok; i++) {
            char* end = nullptr;
            render.matrix[i] = strtof(p, &end);
            ok = end != p && std::isfinite(render.matrix[i]) && fabsf(render.matrix[i]) <= 256.0f && *end == (i < 8 ? ',' : '\0');
            p = end + 1;
        }
        if (!ok) {
            fprintf(stderr, "MFSR_CCM=%s: nine finite coefficients m00,m01,...,m22 with |m| <= 256 expected\n", e);
            return 1;
        }
        ccm = true;
        render.format = MFSR_OUT_RGB8;
        render.useMatrix = 1;
    }
    // MFSR_SHARPEN="amount[,sigma[,radius[,threshold]]]": an unsharp mask inside the finish, on the linear value before the
    // matrix and the tone curve (mfsr_burst_set_sharpen; sigma 1, radius chosen from sigma, threshold 0 by default).  The 8-bit
    // image then comes out of the sharpened finish, with or without MFSR_CCM; _sr2_result stays the sharpenImg2 pass of it.
    bool sharpenOn = false;
    mfsr_sharpen sharpen;
    memset(&sharpen, 0, sizeof(sharpen));
    if (const char* e = getenv("MFSR_SHARPEN")) {
        float v[4] = {0.0f, 1.0f, 0.0f, 0.0f};  // amount, sigma, radius, threshold
        const char* p = e;
        bool ok = true;
        for (int n = 0; ok; n++) {
            char* end = nullptr;
            v[n] = strtof(p, &end);
            ok = end != p && std::isfinite(v[n]);
            p = end;
            if (!ok || *p == '\0') break;
            ok = *p == ',' && n < 3;
            p++;
        }
        ok = ok && *p == '\0' && v[2] >= 0.0f && v[2] <= 4.0f && v[2] == (float)(int)v[2] &&
             mfsr_sharpen_gaussian(v[1], (int)v[2], v[0], v[3], &sharpen) == MFSR_OK;
        if (!ok) {
            fprintf(stderr, "MFSR_SHARPEN=%s: amount[,sigma[,radius[,threshold]]] expected: 0 <= amount <= 16, sigma > 0, radius 0..4, "
                            "threshold >= 0\n", e);
            return 1;
        }
        sharpenOn = true;
        render.format = MFSR_OUT_RGB8;
    }
    // MFSR_DENOISE="strength[,radius[,gain]]": the merge-aware range filter inside the finish, on the linear value before the
    // matrix and the tone curve (mfsr_burst_set_denoise; radius 2, gain 2 by default; alpha and beta are cfg's at the time of the
    // finish, so MFSR_NOISE's measurement goes in).  The 8-bit image then comes out of the denoised finish.
    bool denoiseOn = false;
    mfsr_denoise denoise;
    memset(&denoise, 0, sizeof(denoise));
    if (const char* e = getenv("MFSR_DENOISE")) {
        float v[3] = {0.0f, 2.0f, 2.0f};  // strength, radius, gain
        const char* p = e;
        bool ok = true;
        for (int n = 0; ok; n++) {
            char* end = nullptr;
            v[n] = strtof(p, &end);
            ok = end != p && std::isfinite(v[n]);
            p = end;
            if (!ok || *p == '\0') break;
            ok = *p == ',' && n < 2;
            p++;
        }
        ok = ok && *p == '\0' && v[1] >= 1.0f && v[1] <= 3.0f && v[1] == (float)(int)v[1] && v[0] != 0.0f &&
             mfsr_denoise_defaults(0.0f, 0.0f, &denoise) == MFSR_OK;
        if (ok) {
            denoise.strength = v[0];
            denoise.radius = (int)v[1];
            denoise.gain = v[2];
            ok = mfsr_denoise_validate(&denoise) == MFSR_OK;
        }
        if (!ok) {
            fprintf(stderr, "MFSR_DENOISE=%s: strength[,radius[,gain]] expected: 1/16 <= strength <= 16, radius 1..3, 0 < gain <= 1024\n", e);
            return 1;
        }
        denoiseOn = true;
        render.format = MFSR_OUT_RGB8;
    }
    if (denoiseOn && sharpenOn) {
        fprintf(stderr, "MFSR_DENOISE is not supported with MFSR_SHARPEN (one stencil per finish: DESIGN.md section 2.24)\n");
        return 1;
    }
    // MFSR_AUTO=wb|tone|wb,tone: white-balance gains and / or a tone table measured on the merged image itself
    // (mfsr_burst_auto_render) go into the render description of the finish; with MFSR_CCM the gains
    // multiply that matrix, with MFSR_SHARPEN the measurement is taken before sharpening.  The 8-bit image then comes out of the
    // rendered finish, as with MFSR_CCM.
    bool autoWb = false, autoTone = false;
    if (const char* e = getenv("MFSR_AUTO")) {
        bool ok = *e != '\0';
        for (const char* p = e; ok && *p;) {
            const char* end = strchr(p, ',');
            const size_t n = end ? (size_t)(end - p) : strlen(p);
            if (n == 2 && strncmp(p, "wb", 2) == 0)
                autoWb = true;
            else if (n == 4 && strncmp(p, "tone", 4) == 0)
                autoTone = true;
            else
                ok = false;
            p += n;
            if (*p == ',') ok = ok && *++p != '\0';
        }
        if (!ok) {
            fprintf(stderr, "MFSR_AUTO=%s: wb, tone or wb,tone expected\n", e);
            return 1;
        }
        render.format = MFSR_OUT_RGB8;
    }
    const bool autoOn = autoWb || autoTone;
    // MFSR_LOCAL_TONE="shadows[,highlights[,cell[,bins]]]": local tone mapping inside the finish (mfsr_burst_local_tone, DESIGN.md
    // section 2.25): a bilateral grid of gains measured on the merged image, after MFSR_AUTO's measurement and with its matrix,
    // lifts shadows locally (highlights 0.25, the cell chosen from the frame, 16 bins by default).  The 8-bit image then comes
    // out of the rendered finish, as with MFSR_CCM.
    bool localToneOn = false;
    float localToneV[4] = {0.0f, 0.25f, 0.0f, 16.0f};  // shadows, highlights, cell (0 = default), bins
    if (const char* e = getenv("MFSR_LOCAL_TONE")) {
        const char* p = e;
        bool ok = true;
        for (int n = 0; ok; n++) {
            char* end = nullptr;
            localToneV[n] = strtof(p, &end);
            ok = end != p && std::isfinite(localToneV[n]);
            p = end;
            if (!ok || *p == '\0') break;
            ok = *p == ',' && n < 3;
            p++;
        }
        mfsr_local_tone probe;
        ok = ok && *p == '\0' && localToneV[2] == (float)(int)localToneV[2] && localToneV[3] == (float)(int)localToneV[3] &&
             mfsr_local_tone_defaults(16, 16, &probe) == MFSR_OK;
        if (ok) {
            probe.shadows = localToneV[0];
            probe.highlights = localToneV[1];
            if (localToneV[2] != 0.0f) probe.cell = (int)localToneV[2];
            probe.bins = (int)localToneV[3];
            ok = mfsr_local_tone_validate(&probe) == MFSR_OK;
        }
        if (!ok) {
            fprintf(stderr, "MFSR_LOCAL_TONE=%s: shadows[,highlights[,cell[,bins]]] expected: shadows and highlights in [0, 1], cell a "
                            "power of two 16..512 (0 = chosen from the frame), bins 4, 8, 16 or 32\n", e);
            return 1;
        }
        localToneOn = true;
        render.format = MFSR_OUT_RGB8;
    }
    if (localToneOn && (sharpenOn || denoiseOn)) {
        fprintf(stderr, "MFSR_LOCAL_TONE is not supported with %s (the local-tone finish is pointwise: DESIGN.md section 2.25)\n",
                sharpenOn ? "MFSR_SHARPEN" : "MFSR_DENOISE");
        return 1;
    }
    if (localToneOn && gpus > 1) {
        fprintf(stderr, "MFSR_LOCAL_TONE is not supported with MFSR_GPUS > 1 (the multi-GPU burst gathers 16-bit camera RGB)\n");
        return 1;
    }
    // MFSR_LENS="k1[,k2[,k3[,lateralR,lateralB]]]" / MFSR_OUT_SIZE="WxH": _sr_result comes out of the geometric finish (DESIGN.md
    // section 2.27) at W x H (default: the x2 size) with the lens profile's numbers as they are (default: none), Catmull-Rom.
    // Either alone is allowed.  The description is checked by the library (mfsr_geometry_lens).
    bool geometryOn = false;
    mfsr_geometry geometry;
    {
        const int hrW0 = W * scale, hrH0 = H * scale;
        int gw = hrW0, gh = hrH0;
        double lensK[3] = {0.0, 0.0, 0.0}, lateral[2] = {1.0, 1.0};
        if (const char* e = getenv("MFSR_OUT_SIZE")) {
            char* end = nullptr;
            const long w = strtol(e, &end, 10);
            const bool okW = end != e && *end == 'x';
            const char* p = end + 1;
            const long h = okW ? strtol(p, &end, 10) : 0;
            if (!okW || end == p || *end != '\0' || w < 1 || w > 32768 || h < 1 || h > 32768) {
                fprintf(stderr, "MFSR_OUT_SIZE=%s: WxH expected, 1 <= W, H <= 32768\n", e);
                return 1;
            }
            gw = (int)w;
            gh = (int)h;
            geometryOn = true;
        }
        if (const char* e = getenv("MFSR_LENS")) {
            double v[5] = {0.0, 0.0, 0.0, 1.0, 1.0};
            const char* p = e;
            bool ok = true;
            int n = 0;
            for (; ok; n++) {
                char* end = nullptr;
                v[n] = strtod(p, &end);
                ok = end != p && std::isfinite(v[n]);
                p = end;
                if (!ok || *p == '\0') break;
                ok = *p == ',' && n < 4;
                p++;
            }
            if (!ok || *p != '\0' || n == 3) {  // (n + 1 values: four would be one lateral magnification without the other)
                fprintf(stderr, "MFSR_LENS=%s: k1[,k2[,k3[,lateralR,lateralB]]] expected: |k| <= 4, |lateral - 1| <= 0.25\n", e);
                return 1;
            }
            for (int i = 0; i < 3; i++) lensK[i] = v[i];
            lateral[0] = v[3];
            lateral[1] = v[4];
            geometryOn = true;
        }
        if (geometryOn && mfsr_geometry_lens(hrW0, hrH0, gw, gh, 1.0, lensK, lateral, MFSR_GEO_CUBIC, &geometry) != MFSR_OK) {
            fprintf(stderr, "MFSR_LENS / MFSR_OUT_SIZE: |k| <= 4, |lateral - 1| <= 0.25 and an output between 1/8 and 8 times the x%d size "
                            "expected\n", scale);
            return 1;
        }
    }
    if (geometryOn && (sharpenOn || denoiseOn || localToneOn)) {
        fprintf(stderr, "MFSR_LENS / MFSR_OUT_SIZE is not supported with %s (the geometric finish knows no other stage: DESIGN.md section "
                        "2.27)\n", sharpenOn ? "MFSR_SHARPEN" : (denoiseOn ? "MFSR_DENOISE" : "MFSR_LOCAL_TONE"));
        return 1;
    }
    if (geometryOn && gpus > 1) {
        fprintf(stderr, "MFSR_LENS / MFSR_OUT_SIZE is not supported with MFSR_GPUS > 1 (the multi-GPU burst gathers 16-bit camera RGB)\n");
        return 1;
    }
    if (geometryOn) render.format = MFSR_OUT_RGB8;
    // the 8-bit image comes out of the finish launch
    const bool rendered = ccm || sharpenOn || denoiseOn || autoOn || localToneOn || geometryOn;
    if (denoiseOn && gpus > 1) {
        fprintf(stderr, "MFSR_DENOISE is not supported with MFSR_GPUS > 1 (the multi-GPU burst gathers 16-bit camera RGB)\n");
        return 1;
    }
    if (autoOn && gpus > 1) {
        fprintf(stderr, "MFSR_AUTO is not supported with MFSR_GPUS > 1 (the multi-GPU burst gathers 16-bit camera RGB)\n");
        return 1;
    }
    if (sharpenOn && gpus > 1) {
        fprintf(stderr, "MFSR_SHARPEN is not supported with MFSR_GPUS > 1 (the multi-GPU burst gathers 16-bit camera RGB)\n");
        return 1;
    }
    if (ccm && gpus > 1) {
        fprintf(stderr, "MFSR_CCM is not supported with MFSR_GPUS > 1 (the multi-GPU burst gathers 16-bit camera RGB)\n");
        return 1;
    }
    if (noiseMode && gpus > 1) {
        fprintf(stderr, "MFSR_NOISE is not supported with MFSR_GPUS > 1 (calibrate on one GPU and pass the values)\n");
        return 1;
    }
    if (exposure && gpus > 1) {
        fprintf(stderr, "MFSR_EXPOSURE is not supported with MFSR_GPUS > 1 (match the frames before sharding them)\n");
        return 1;
    }
    if (!shadingMap.empty() && gpus > 1) {
        fprintf(stderr, "MFSR_SHADING is not supported with MFSR_GPUS > 1 (correct the frames before sharding them)\n");
        return 1;
    }
    if (defects && gpus > 1) {
        fprintf(stderr, "MFSR_DEFECTS is not supported with MFSR_GPUS > 1 (each rank holds only its own frames)\n");
        return 1;
    }
    if (selectCandidates >= 0 && gpus > 1) {
        fprintf(stderr, "MFSR_SELECT is not supported with MFSR_GPUS > 1 (the multi-GPU burst takes frame 0 as its reference)\n");
        return 1;
    }
    if (gpus > 1) {
        // ---- the burst sharded over `gpus` GPUs from this one process ------------------------------------------------
        const bool virt = getenv("MFSR_VIRTUAL_RANKS") && getenv("MFSR_VIRTUAL_RANKS")[0] == '1';
        if (!virt && mfsr_device_count() < gpus) {
            fprintf(stderr, "MFSR_GPUS=%d but only %d HIP device(s) are visible\n", gpus, mfsr_device_count());
            return 1;
        }
        std::vector<int> devs(gpus);
        for (int r = 0; r < gpus; r++) devs[r] = virt ? 0 : r;
        const size_t dwsBytes = mfsr_dist_workspace_bytes(&cfg, gpus);
        if (!dwsBytes) {
            fprintf(stderr, "mfsr_dist_workspace_bytes: invalid configuration\n");
            return 1;
        }
        std::vector<void*> dws(gpus, nullptr);
        std::vector<const uint16_t*> table((size_t)gpus * num_images, nullptr);  // row r: rank r's frames + the reference
        std::vector<int*> dstatus(gpus, nullptr);
        for (int r = 0; r < gpus; r++) {
            HIP_OK(hipSetDevice(devs[r]));
            HIP_OK(hipMalloc(&dws[r], dwsBytes));
            HIP_OK(hipMalloc((void**)&dstatus[r], sizeof(int)));
            for (int k = 0; k < num_images; k++) {
                if (k % gpus != r && k != cfg.reference) continue;
                uint16_t* p = nullptr;
                HIP_OK(hipMalloc((void**)&p, (size_t)W * H * 2));
                HIP_OK(hipMemcpy(p, raws[k].data(), (size_t)W * H * 2, hipMemcpyHostToDevice));  // :172 upload
                table[(size_t)r * num_images + k] = p;
            }
        }
        HIP_OK(hipSetDevice(devs[0]));
        uint16_t* d16 = nullptr;
        HIP_OK(hipMalloc((void**)&d16, (size_t)hrW * hrH * 6));
        mfsr_dist_group* g = nullptr;
        MFSR_OK_OR_DIE(mfsr_dist_group_create(&g, &cfg, gpus, devs.data(), dws.data(), dwsBytes));
        bool wholeFrames = false;
        for (int rep = 0; rep < num_times; rep++) {
            if (rep == start_i) {
                MFSR_OK_OR_DIE(mfsr_dist_group_synchronize(g, nullptr));
                t0 = std::chrono::steady_clock::now();
            }
            MFSR_OK_OR_DIE(mfsr_dist_group_process_burst(g, table.data(), MFSR_DIST_STRIPES, d16, dstatus.data(), nullptr));
            if (rep == 0 && !wholeFrames) {  // a flow beyond the raw halo of the stripe exchange: exchange whole raw frames
                MFSR_OK_OR_DIE(mfsr_dist_group_synchronize(g, nullptr));
                int st = 0;
                HIP_OK(hipMemcpy(&st, dstatus[0], sizeof(int), hipMemcpyDeviceToHost));
                if (st != 0) {
                    MFSR_OK_OR_DIE(mfsr_dist_group_set_raw_halo(g, H));
                    wholeFrames = true;
                    rep = -1;
                }
            }
        }
        MFSR_OK_OR_DIE(mfsr_dist_group_synchronize(g, nullptr));
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%g sec\n", sec);                                               // :205
        printf("%g FPS\n", (double)(num_images * real_times) / sec);           // :206
        std::vector<uint16_t> h16((size_t)hrW * hrH * 3);
        HIP_OK(hipMemcpy(h16.data(), d16, h16.size() * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h16.size(); i++) h8[i] = (uint8_t)(((unsigned)h16[i] * 255u + 32767u) / 65535u);
        HIP_OK(hipMalloc((void**)&d8, h8.size()));
        HIP_OK(hipMalloc((void**)&d8s, h8.size()));
        HIP_OK(hipMemcpy(d8, h8.data(), h8.size(), hipMemcpyHostToDevice));
        MFSR_OK_OR_DIE(mfsr_sharpenImg2(d8, d8s, hrH, hrW, 3, hrW * 3, hrW * 3, nullptr));
        HIP_OK(hipMemcpy(h8s.data(), d8s, h8s.size(), hipMemcpyDeviceToHost));
        mfsr_dist_group_destroy(g);
        if (!write_png(inputName + "_" + optFlowName + "_sr_result.png", h8.data(), hrW, hrH, 3) ||   // :207
            !write_png(inputName + "_" + optFlowName + "_sr2_result.png", h8s.data(), hrW, hrH, 3)) {  // :209
            fprintf(stderr, "cannot write result PNGs\n");
            return 1;
        }
        return 0;
    }

    const size_t wsBytes = mfsr_burst_workspace_bytes(&cfg), accBytes = mfsr_burst_accumulator_bytes(&cfg);
    void *ws = nullptr, *imgOut = nullptr, *weights = nullptr, *outF = nullptr;
    HIP_OK(hipMalloc(&ws, wsBytes));
    HIP_OK(hipMalloc(&imgOut, accBytes));
    HIP_OK(hipMalloc(&weights, accBytes));
    HIP_OK(hipMalloc(&outF, accBytes));
    std::vector<uint16_t*> dframes(num_images);
    for (int k = 0; k < num_images; k++) {
        HIP_OK(hipMalloc((void**)&dframes[k], (size_t)W * H * 2));
        HIP_OK(hipMemcpy(dframes[k], raws[k].data(), (size_t)W * H * 2, hipMemcpyHostToDevice));  // :172 upload
    }
    mfsr_burst* b = nullptr;
    MFSR_OK_OR_DIE(mfsr_burst_create(&b, &cfg, ws, wsBytes));

    // MFSR_DEFECTS: repaired once, in the device frames, before the selection and before the replays
    // (mfsr_burst_repair_defects); the report goes to stderr so that stdout stays the reference's
    if (defects) {
        uint8_t* dmap = nullptr;
        uint32_t* dcounts = nullptr;
        uint32_t counts[2] = {0, 0};
        HIP_OK(hipMalloc((void**)&dmap, (size_t)W * H));
        HIP_OK(hipMalloc((void**)&dcounts, 2 * sizeof(uint32_t)));
        MFSR_OK_OR_DIE(mfsr_burst_repair_defects(b, num_images, dframes.data(), defThreshold, defSpread, defVotes, dmap, dcounts,
                                                 counts, nullptr));
        HIP_OK(hipFree(dmap));
        HIP_OK(hipFree(dcounts));
        fprintf(stderr, "defects: %u hot, %u cold\n", counts[0], counts[1]);
    }

    // MFSR_SHADING: the gain map applied once, in the device frames, after the repair and before the selection
    // (mfsr_burst_correct_shading); the report goes to stderr
    if (!shadingMap.empty()) {
        int32_t* dmapQ16 = nullptr;
        HIP_OK(hipMalloc((void**)&dmapQ16, shadingMap.size() * sizeof(int32_t)));
        HIP_OK(hipMemcpy(dmapQ16, shadingMap.data(), shadingMap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        MFSR_OK_OR_DIE(mfsr_burst_correct_shading(b, num_images, dframes.data(), dmapQ16, shadingCell, nullptr));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(dmapQ16));
        fprintf(stderr, "shading: map %dx%d cell %d\n", shadingGw, shadingGh, shadingCell);
    }

    // MFSR_SELECT: the sharpest frame becomes the reference and frames much softer than it are dropped, chosen once for the
    // burst before the replays (mfsr_burst_select_frames); the report goes to stderr so that stdout stays the reference's
    int reference = cfg.reference;
    std::vector<int> ids;
    for (int k = 0; k < num_images; k++) ids.push_back(k);
    if (selectCandidates >= 0) {
        long long* dsums = nullptr;
        std::vector<int32_t> keep(num_images);
        HIP_OK(hipMalloc((void**)&dsums, sizeof(long long) * num_images));
        MFSR_OK_OR_DIE(mfsr_burst_select_frames(b, num_images, dframes.data(), selectCandidates, keepRatio, dsums, &reference,
                                                keep.data(), nullptr, nullptr, nullptr));
        HIP_OK(hipFree(dsums));
        ids.clear();
        for (int k = 0; k < num_images; k++)
            if (keep[k]) ids.push_back(k);
        fprintf(stderr, "reference %d, kept %d of %d\n", reference, (int)ids.size(), num_images);
    }

    // MFSR_EXPOSURE: every frame's brightness matched to the reference's, once, in the device frames, after the repair and
    // the selection and before the replays (mfsr_burst_match_exposure); the report goes to stderr
    if (exposure) {
        long long* dlevels = nullptr;
        int32_t deadband = 0, minGain = 0, maxGain = 0;
        std::vector<int32_t> gains(3 * (size_t)num_images), status(num_images);
        HIP_OK(hipMalloc((void**)&dlevels, 5 * sizeof(long long) * num_images));
        MFSR_OK_OR_DIE(mfsr_exposure_defaults(&cfg, nullptr, nullptr, nullptr, &deadband, &minGain, &maxGain, nullptr));
        MFSR_OK_OR_DIE(mfsr_burst_match_exposure(b, num_images, dframes.data(), reference, exposure == 2, deadband, minGain, maxGain,
                                                 dlevels, gains.data(), status.data(), nullptr, nullptr));
        HIP_OK(hipFree(dlevels));
        for (int k = 0; k < num_images; k++)
            fprintf(stderr, "exposure: frame %d gain %d %d %d status %d\n", k, gains[3 * k], gains[3 * k + 1], gains[3 * k + 2], status[k]);
    }

    // MFSR_NOISE=auto: the noise model measured on the (repaired, matched) device frames; alpha and beta are construction-time
    // configuration, so the burst is created again with them (mfsr_burst_calibrate_noise changes nothing itself)
    if (noiseMode == 1) {
        void* dscratch = nullptr;
        float a = 0.0f, bt = 0.0f;
        int32_t st = 0;
        HIP_OK(hipMalloc(&dscratch, MFSR_NOISE_SCRATCH_BYTES));
        MFSR_OK_OR_DIE(mfsr_burst_calibrate_noise(b, num_images, dframes.data(), dscratch, &a, &bt, &st, nullptr));
        HIP_OK(hipFree(dscratch));
        fprintf(stderr, "noise: alpha %g beta %g status %d\n", a, bt, st);
        if (st == 0) {
            cfg.alpha = a;
            cfg.beta = bt;
            mfsr_burst_destroy(b);
            b = nullptr;
            MFSR_OK_OR_DIE(mfsr_burst_create(&b, &cfg, ws, wsBytes));
        }
    }

    // MFSR_NOISE=burst: the noise model measured on the burst being processed -- the kept (repaired, shaded, matched) frames
    // aligned to the reference through a handle of its own, which is thrown away: the burst below starts on a fresh one, with
    // the measured values when the status is 0 (mfsr_burst_calibrate_noise_temporal)
    if (noiseMode == 3) {
        std::vector<const uint16_t*> kept;
        int refAt = -1;
        for (int k : ids) {
            if (k == reference) refAt = (int)kept.size();
            kept.push_back(dframes[k]);
        }
        double a = 0.0, bt = 0.0;
        int32_t st = 2, pts = 0;
        long long terms = 0;
        const size_t need = mfsr_noise_temporal_scratch_bytes(&cfg, (int)kept.size());
        if (need != 0 && refAt >= 0) {
            void* dscratch = nullptr;
            HIP_OK(hipMalloc(&dscratch, need));
            HIP_OK(hipDeviceSynchronize());  // (the raw-domain steps above are through with the first handle)
            mfsr_burst_destroy(b);
            b = nullptr;
            mfsr_burst* cal = nullptr;
            MFSR_OK_OR_DIE(mfsr_burst_create(&cal, &cfg, ws, wsBytes));
            MFSR_OK_OR_DIE(mfsr_burst_calibrate_noise_temporal(cal, (int)kept.size(), kept.data(), refAt, 0.0f, 0, dscratch, need, &a, &bt,
                                                               &st, &pts, &terms, nullptr));
            mfsr_burst_destroy(cal);
            HIP_OK(hipFree(dscratch));
            if (st == 0) {
                cfg.alpha = (float)a;
                cfg.beta = (float)bt;
            }
            MFSR_OK_OR_DIE(mfsr_burst_create(&b, &cfg, ws, wsBytes));
        }
        fprintf(stderr, "noise: alpha %g beta %g status %d points %d blocks %lld\n", a, bt, st, pts, terms);
    }

    HIP_OK(hipMalloc((void**)&d8, (size_t)hrW * hrH * 3));
    HIP_OK(hipMalloc((void**)&d8s, (size_t)hrW * hrH * 3));
    uint8_t* d8g = nullptr;  // MFSR_LENS / MFSR_OUT_SIZE: the geometric finish's 8-bit image
    if (geometryOn) HIP_OK(hipMalloc((void**)&d8g, (size_t)geometry.outW * geometry.outH * 3));
    if (rendered) MFSR_OK_OR_DIE(mfsr_burst_set_render(b, &render));
    if (sharpenOn) MFSR_OK_OR_DIE(mfsr_burst_set_sharpen(b, &sharpen));
    if (denoiseOn) {
        denoise.alpha = cfg.alpha;  // (as calibrated, when MFSR_NOISE asked for it)
        denoise.beta = cfg.beta;
        MFSR_OK_OR_DIE(mfsr_burst_set_denoise(b, &denoise));
    }
    // MFSR_AUTO: the table of the statistics and the tone table the measurement writes (device memory of the caller's)
    uint64_t* dstats = nullptr;
    float* dlut = nullptr;
    mfsr_auto_params autoParams;
    mfsr_auto_result autoResult;
    memset(&autoResult, 0, sizeof(autoResult));
    if (autoOn) {
        MFSR_OK_OR_DIE(mfsr_auto_defaults((long long)hrW * hrH, &autoParams));
        autoParams.awb = autoWb;
        autoParams.tone = autoTone;
        HIP_OK(hipMalloc((void**)&dstats, sizeof(uint64_t) * MFSR_IMAGE_STATS_WORDS));
        HIP_OK(hipMalloc((void**)&dlut, sizeof(float) * ((size_t)autoParams.toneSize + 1)));
    }
    // MFSR_LOCAL_TONE: the description for this frame, the statistics table and the grid (device memory of the caller's)
    mfsr_local_tone localTone;
    mfsr_local_tone_result localToneResult;
    memset(&localToneResult, 0, sizeof(localToneResult));
    uint64_t* dtoneStats = nullptr;
    float* dtoneGrid = nullptr;
    if (localToneOn) {
        MFSR_OK_OR_DIE(mfsr_local_tone_defaults(hrW, hrH, &localTone));
        localTone.shadows = localToneV[0];
        localTone.highlights = localToneV[1];
        if (localToneV[2] != 0.0f) localTone.cell = (int)localToneV[2];
        localTone.bins = (int)localToneV[3];
        int gx = 0, gy = 0, gz = 0;
        MFSR_OK_OR_DIE(mfsr_local_tone_grid(hrW, hrH, &localTone, &gx, &gy, &gz));
        HIP_OK(hipMalloc((void**)&dtoneStats, sizeof(uint64_t) * 2 * (size_t)gx * gy * gz));
        HIP_OK(hipMalloc((void**)&dtoneGrid, sizeof(float) * (size_t)gx * gy * gz));
    }
    for (int rep = 0; rep < num_times; rep++) {
        if (rep == start_i) {
            HIP_OK(hipDeviceSynchronize());
            t0 = std::chrono::steady_clock::now();  // tm1.start(), :188-190
        }
        HIP_OK(hipMemsetAsync(imgOut, 0, accBytes, nullptr));
        HIP_OK(hipMemsetAsync(weights, 0, accBytes, nullptr));
        MFSR_OK_OR_DIE(mfsr_burst_set_reference(b, dframes[reference], nullptr));
        for (int k : ids)
            MFSR_OK_OR_DIE(mfsr_burst_add_frame(b, dframes[k], k == reference, (mfsr_float3*)imgOut,
                                                (mfsr_float3*)weights, nullptr));
        if (autoOn) {  // measured on this burst's accumulators; the description it installs is the one the finish below uses
            mfsr_render measured = render;
            MFSR_OK_OR_DIE(mfsr_burst_auto_render(b, (const mfsr_float3*)imgOut, (const mfsr_float3*)weights, &autoParams, dstats, dlut,
                                                  &measured, &autoResult, nullptr));
        }
        if (localToneOn)  // after the auto render: measured with the matrix the finish below uses
            MFSR_OK_OR_DIE(mfsr_burst_local_tone(b, (const mfsr_float3*)imgOut, (const mfsr_float3*)weights, &localTone, dtoneStats,
                                                 dtoneGrid, &localToneResult, nullptr));
        if (rendered)  // (sharpening +) matrix + gamma + 8-bit store in the finish launch: the float image is neither written nor
                       // read again
            MFSR_OK_OR_DIE(mfsr_burst_finish(b, (const mfsr_float3*)imgOut, (const mfsr_float3*)weights,
                                             cfg.fused ? nullptr : (mfsr_float3*)outF, (uint16_t*)d8, nullptr));
        else
            MFSR_OK_OR_DIE(mfsr_burst_finish(b, (const mfsr_float3*)imgOut, (const mfsr_float3*)weights, (mfsr_float3*)outF,
                                             nullptr, nullptr));
        if (geometryOn)  // _sr_result: one more launch on the same accumulators, with the same render description
            MFSR_OK_OR_DIE(mfsr_burst_finish_geometry(b, (const mfsr_float3*)imgOut, (const mfsr_float3*)weights, &geometry, nullptr, 0,
                                                      d8g, 3 * geometry.outW, nullptr));
    }
    HIP_OK(hipDeviceSynchronize());
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%g sec\n", sec);                                               // :205
    printf("%g FPS\n", (double)(num_images * real_times) / sec);           // :206
    if (autoOn)
        fprintf(stderr, "auto: gains %g %g %g (status %d, neutral share %g) black %g white %g gamma %g (status %d)\n",
                autoResult.gains[0], autoResult.gains[1], autoResult.gains[2], autoResult.awbStatus, autoResult.neutralShare,
                autoResult.black, autoResult.white, autoResult.gamma, autoResult.toneStatus);
    if (localToneOn)
        fprintf(stderr, "local tone: cell %d bins %d pivot %g gains %g .. %g (status %d)\n", localTone.cell, localTone.bins,
                localToneResult.pivot, localToneResult.minGain, localToneResult.maxGain, localToneResult.status);

    // result -> 8-bit RGB (D2H), then sharpenImg2 on the device
    if (!rendered) MFSR_OK_OR_DIE(mfsr_quantize((const mfsr_float3*)outF, 12 * hrW, nullptr, d8, hrW, hrH, 255.0f, nullptr));
    MFSR_OK_OR_DIE(mfsr_sharpenImg2(d8, d8s, hrH, hrW, 3, hrW * 3, hrW * 3, nullptr));
    HIP_OK(hipMemcpy(h8.data(), d8, h8.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h8s.data(), d8s, h8s.size(), hipMemcpyDeviceToHost));
    std::vector<uint8_t> h8g;
    if (geometryOn) {
        h8g.resize((size_t)geometry.outW * geometry.outH * 3);
        HIP_OK(hipMemcpy(h8g.data(), d8g, h8g.size(), hipMemcpyDeviceToHost));
    }
    if (!(geometryOn ? write_png(inputName + "_" + optFlowName + "_sr_result.png", h8g.data(), geometry.outW, geometry.outH, 3)
                     : write_png(inputName + "_" + optFlowName + "_sr_result.png", h8.data(), hrW, hrH, 3)) ||  // :207
        !write_png(inputName + "_" + optFlowName + "_sr2_result.png", h8s.data(), hrW, hrH, 3)) {  // :209
        fprintf(stderr, "cannot write result PNGs\n");
        return 1;
    }
    mfsr_burst_destroy(b);
    return 0;
}
