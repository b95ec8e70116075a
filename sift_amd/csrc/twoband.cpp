// Host side of the two-band compositor (include/sift_hip.h: sift_hip_composite_twoband): checks, staging of caller memory and the
// scratch memory, which the first call of a context allocates and the context keeps - outside the batch arena, like the
// compositor's.  The kernel: kernels_twoband.hip; the definition: twoband_math.h.
#include <climits>
#include <cstring>
#include <string>

#include "common.h"
#include "twoband_kernels.h"
#include "twoband_math.h"   // kWarpMaxSide, kCompositeMaxJobs, the taps' conditions and the constant norm

namespace sift_hip {

struct TwobandState {
    ScratchBuf d_imgs, d_models, d_src, d_offsets, d_gains;   // what arrives in host memory
    ScratchBuf d_out, d_count;                                // results on their way to host memory
    ScratchBuf d_tiles;                                       // the three visit counters
};

void twoband_state_free(TwobandState* st) {
    if (!st) return;
    for (ScratchBuf* b : {&st->d_imgs, &st->d_models, &st->d_src, &st->d_offsets, &st->d_gains, &st->d_out, &st->d_count, &st->d_tiles}) b->release();
    delete st;
}

namespace {

struct Job {
    sift_hip_ctx* c;
    const float* imgs;
    int n_imgs, w, h, n_canvases;
    const int64_t* offsets;
    const int32_t* src;
    const float* models;
    const sift_hip_twoband_params* p;
    const float* taps;
    const float* gains;   // one per job, host or device memory; null: none
    float* out;
    uint16_t* count;
    int64_t* tiles;
    char* err;
    int errlen;
};

int fail(const Job& j, const char* msg) {
    match_set_err(j.err, j.errlen, (std::string("sift_hip_composite_twoband: ") + msg).c_str());
    return SIFT_HIP_EINVAL;
}

int run(void* arg) {
    const Job& j = *static_cast<const Job*>(arg);
    const sift_hip_twoband_params* p = j.p;
    if (!p) return fail(j, "no parameters");
    if (j.n_imgs < 1 || j.w < 1 || j.h < 1 || j.w > kWarpMaxSide || j.h > kWarpMaxSide) return fail(j, "images are n_imgs >= 1 of 1 .. 2^22 pixels a side");
    if (j.n_canvases < 0 || j.n_canvases > 65535) return fail(j, "n_canvases must be 0 .. 65535");
    if (p->out_w < 1 || p->out_h < 1) return fail(j, "out_w and out_h must be > 0");
    if (p->radius > kTwobandMaxRadius) return fail(j, "radius must be 0 .. 16");
    const long long lim = 1ll << 24, R = p->radius;   // the window reaches R lattice points beyond the canvas
    if ((long long)p->origin_x - R <= -lim || (long long)p->origin_x + p->out_w - 1 + R >= lim || (long long)p->origin_y - R <= -lim ||
        (long long)p->origin_y + p->out_h - 1 + R >= lim)
        return fail(j, "a lattice coordinate of the canvas widened by the radius reaches 2^24 in magnitude");
    if (p->interp > 1) return fail(j, "interp must be 0 (nearest) or 1 (bilinear)");
    if (p->path > 1) return fail(j, "path must be 0 or 1");
    if (p->reserved) return fail(j, "the reserved byte must be zero");
    if (!j.taps) return fail(j, "a null argument");
    if (!twoband_taps_ok(j.taps, p->radius)) return fail(j, "taps must be finite and >= 0, the centre tap >= 2^-12");
    if (j.n_canvases == 0) return SIFT_HIP_OK;
    if (!j.offsets || !j.imgs || !j.out) return fail(j, "a null argument");
    if (j.offsets[0] != 0) return fail(j, "offsets must start at 0");
    for (int c = 0; c < j.n_canvases; ++c) {
        if (j.offsets[c + 1] < j.offsets[c]) return fail(j, "offsets must not decrease");
        if (j.offsets[c + 1] - j.offsets[c] > kCompositeMaxJobs) return fail(j, "more than 65535 jobs in one canvas");
    }
    const int64_t n_jobs = j.offsets[j.n_canvases];
    if (n_jobs > INT_MAX) return fail(j, "more than 2^31 - 1 jobs");
    if (n_jobs > 0 && !j.models) return fail(j, "a null argument");
    if (!j.src && n_jobs > j.n_imgs) return fail(j, "without src, job j reads image j: more jobs than images");
    if (j.src)
        for (int64_t k = 0; k < n_jobs; ++k)
            if (j.src[k] < 0 || j.src[k] >= j.n_imgs) return fail(j, "a src index outside the images");

    const MatchCtxView v = match_ctx_view(j.c);
    SIFT_HIP_CHECK(hipSetDevice(v.device));
    TwobandState** slot = twoband_ctx_state(j.c);
    if (!*slot) *slot = new TwobandState();
    TwobandState& st = **slot;

    // ---- inputs on the device ----
    const size_t img_bytes = (size_t)j.n_imgs * (size_t)j.w * (size_t)j.h * sizeof(float), model_bytes = (size_t)n_jobs * 9 * sizeof(float);
    const size_t px = (size_t)j.n_canvases * (size_t)p->out_w * (size_t)p->out_h;
    const float* d_imgs = j.imgs;
    if (!match_ptr_on_device(j.imgs)) {
        st.d_imgs.ensure(img_bytes);
        match_upload(j.c, st.d_imgs.p, j.imgs, img_bytes);
        match_wait(j.c);   // pageable memory travels through the context's two staging buffers: the next upload refills them
        d_imgs = st.d_imgs.as<float>();
    }
    const float* d_models = j.models;
    if (n_jobs > 0 && !match_ptr_on_device(j.models)) {
        st.d_models.ensure(model_bytes);
        match_upload(j.c, st.d_models.p, j.models, model_bytes);
        match_wait(j.c);
        d_models = st.d_models.as<float>();
    }
    const int* d_src = nullptr;
    if (j.src && n_jobs > 0) {
        st.d_src.ensure((size_t)n_jobs * sizeof(int));
        match_upload(j.c, st.d_src.p, j.src, (size_t)n_jobs * sizeof(int));
        match_wait(j.c);
        d_src = st.d_src.as<int>();
    }
    const size_t off_bytes = ((size_t)j.n_canvases + 1) * sizeof(int64_t);
    st.d_offsets.ensure(off_bytes);
    match_upload(j.c, st.d_offsets.p, j.offsets, off_bytes);
    match_wait(j.c);
    const float* d_gains = n_jobs > 0 ? j.gains : nullptr;
    if (d_gains && !match_ptr_on_device(j.gains)) {
        st.d_gains.ensure((size_t)n_jobs * sizeof(float));
        match_upload(j.c, st.d_gains.p, j.gains, (size_t)n_jobs * sizeof(float));
        match_wait(j.c);
        d_gains = st.d_gains.as<float>();
    }

    // ---- results: written in place when the caller's array is device memory ----
    const bool out_direct = match_ptr_on_device(j.out), count_direct = j.count && match_ptr_on_device(j.count);
    if (!out_direct) st.d_out.ensure(px * sizeof(float));
    if (j.count && !count_direct) st.d_count.ensure(px * sizeof(uint16_t));
    float* d_out = out_direct ? j.out : st.d_out.as<float>();
    uint16_t* d_count = !j.count ? nullptr : (count_direct ? j.count : st.d_count.as<uint16_t>());
    unsigned long long* d_tiles = nullptr;
    if (j.tiles) {
        st.d_tiles.ensure(256);
        d_tiles = st.d_tiles.as<unsigned long long>();
        launch_zero_ints(v.stream, st.d_tiles.as<int>(), 6);
    }

    // the taps travel in the kernel's arguments, with the one ln of a fully covered window (the same header, the same bits)
    TwobandArgs a{p->out_w, p->out_h, p->origin_x, p->origin_y, p->fill, (int)p->interp, (int)p->path, (int)p->radius, twoband_full_norm(j.taps, p->radius), {}};
    std::memcpy(a.taps, j.taps, ((size_t)p->radius + 1) * sizeof(float));
    launch_twoband(v.stream, d_imgs, j.w, j.h, d_src, d_models, st.d_offsets.as<long long>(), j.n_canvases, a, d_out, d_count, d_tiles, d_gains);
    SIFT_HIP_CHECK(hipGetLastError());

    if (!out_direct) match_download(j.c, j.out, d_out, px * sizeof(float));
    if (j.count && !count_direct) match_download(j.c, j.count, d_count, px * sizeof(uint16_t));
    if (j.tiles) match_download(j.c, j.tiles, d_tiles, 3 * sizeof(int64_t));
    match_wait(j.c);
    return SIFT_HIP_OK;
}

}  // namespace
}  // namespace sift_hip

using namespace sift_hip;

extern "C" int sift_hip_composite_twoband(sift_hip_ctx* c, const float* imgs, int n_imgs, int w, int h, int n_canvases, const int64_t* offsets,
                                          const int32_t* src, const float* models, const sift_hip_twoband_params* params, const float* taps,
                                          const float* gains, float* out, uint16_t* count, int64_t* tiles, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_composite_twoband: no context (the two-band compositor runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, imgs, n_imgs, w, h, n_canvases, offsets, src, models, params, taps, gains, out, count, tiles, err, errlen};
    return match_guarded(err, errlen, run, &j);
}
