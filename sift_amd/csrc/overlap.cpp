// Host side of the overlap statistics (include/sift_hip.h: sift_hip_overlap_stats): checks, staging of caller memory and the
// scratch memory, which the first call of a context allocates and the context keeps - outside the batch arena, like the
// compositor's.  The kernels: kernels_overlap.hip; the definition: overlap_math.h.
#include <climits>
#include <cstring>
#include <string>

#include "common.h"
#include "overlap_kernels.h"
#include "overlap_math.h"   // kWarpMaxSide, kOverlapMaxJobs

namespace sift_hip {

struct OverlapState {
    ScratchBuf d_imgs, d_models, d_src, d_offsets;   // what arrives in host memory
    ScratchBuf d_stats, d_gains, d_status;           // results on their way to host memory
};

void overlap_state_free(OverlapState* st) {
    if (!st) return;
    for (ScratchBuf* b : {&st->d_imgs, &st->d_models, &st->d_src, &st->d_offsets, &st->d_stats, &st->d_gains, &st->d_status}) b->release();
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
    const sift_hip_overlap_params* p;
    int64_t* stats;
    float* gains;
    uint8_t* status;
    char* err;
    int errlen;
};

int fail(const Job& j, const char* msg) {
    match_set_err(j.err, j.errlen, (std::string("sift_hip_overlap_stats: ") + msg).c_str());
    return SIFT_HIP_EINVAL;
}

bool positive(float v) { return v > 0.0f && v - v == 0.0f; }   // finite and > 0

int run(void* arg) {
    const Job& j = *static_cast<const Job*>(arg);
    const sift_hip_overlap_params* p = j.p;
    if (!p) return fail(j, "no parameters");
    if (j.n_imgs < 1 || j.w < 1 || j.h < 1 || j.w > kWarpMaxSide || j.h > kWarpMaxSide) return fail(j, "images are n_imgs >= 1 of 1 .. 2^22 pixels a side");
    if (j.n_canvases < 0 || j.n_canvases > 65535) return fail(j, "n_canvases must be 0 .. 65535");
    if (p->out_w < 1 || p->out_h < 1) return fail(j, "out_w and out_h must be > 0");
    const long long lim = 1ll << 24;
    if ((long long)p->origin_x <= -lim || (long long)p->origin_x + p->out_w - 1 >= lim || (long long)p->origin_y <= -lim ||
        (long long)p->origin_y + p->out_h - 1 >= lim)
        return fail(j, "a lattice coordinate x + origin_x or y + origin_y reaches 2^24 in magnitude");
    if (p->interp > 1) return fail(j, "interp must be 0 (nearest) or 1 (bilinear)");
    if (p->path > 1) return fail(j, "path must be 0 or 1");
    if (p->reserved[0] || p->reserved[1]) return fail(j, "the reserved bytes must be zero");
    if (!positive(p->scale)) return fail(j, "scale must be finite and > 0");
    if (j.gains && (!positive(p->sigma_n) || !positive(p->sigma_g))) return fail(j, "sigma_n and sigma_g must be finite and > 0");
    if (j.n_canvases == 0) return SIFT_HIP_OK;
    if (!j.offsets || !j.imgs || !j.stats) return fail(j, "a null argument");
    if (j.offsets[0] != 0) return fail(j, "offsets must start at 0");
    for (int c = 0; c < j.n_canvases; ++c) {
        if (j.offsets[c + 1] < j.offsets[c]) return fail(j, "offsets must not decrease");
        if (j.offsets[c + 1] - j.offsets[c] > kOverlapMaxJobs) return fail(j, "more than 32 jobs in one canvas");
    }
    const int64_t n_jobs = j.offsets[j.n_canvases];
    if (n_jobs > 0 && !j.models) return fail(j, "a null argument");
    if (!j.src && n_jobs > j.n_imgs) return fail(j, "without src, job j reads image j: more jobs than images");
    if (j.src)
        for (int64_t k = 0; k < n_jobs; ++k)
            if (j.src[k] < 0 || j.src[k] >= j.n_imgs) return fail(j, "a src index outside the images");

    const MatchCtxView v = match_ctx_view(j.c);
    SIFT_HIP_CHECK(hipSetDevice(v.device));
    OverlapState** slot = overlap_ctx_state(j.c);
    if (!*slot) *slot = new OverlapState();
    OverlapState& st = **slot;

    // ---- inputs on the device ----
    const size_t img_bytes = (size_t)j.n_imgs * (size_t)j.w * (size_t)j.h * sizeof(float), model_bytes = (size_t)n_jobs * 9 * sizeof(float);
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

    // ---- results: written in place when the caller's array is device memory ----
    const size_t stat_bytes = (size_t)j.n_canvases * kOverlapStats * sizeof(int64_t), gain_bytes = (size_t)n_jobs * sizeof(float);
    const bool want_gains = j.gains && n_jobs > 0;
    const bool stats_direct = match_ptr_on_device(j.stats), gains_direct = want_gains && match_ptr_on_device(j.gains);
    const bool status_direct = j.status && match_ptr_on_device(j.status);
    if (!stats_direct) st.d_stats.ensure(stat_bytes);
    if (want_gains && !gains_direct) st.d_gains.ensure(gain_bytes);
    if (!status_direct) st.d_status.ensure((size_t)j.n_canvases);   // the kernel's own when the caller wants none
    long long* d_stats = stats_direct ? reinterpret_cast<long long*>(j.stats) : st.d_stats.as<long long>();
    float* d_gains = gains_direct ? j.gains : st.d_gains.as<float>();
    uint8_t* d_status = status_direct ? j.status : st.d_status.as<uint8_t>();

    launch_zero_ints(v.stream, reinterpret_cast<int*>(d_stats), stat_bytes / sizeof(int));
    const OverlapArgs a{p->out_w, p->out_h, p->origin_x, p->origin_y, p->scale, (int)p->interp, (int)p->path};
    launch_overlap_stats(v.stream, d_imgs, j.w, j.h, d_src, d_models, st.d_offsets.as<long long>(), j.n_canvases, a, d_stats);
    if (want_gains) launch_overlap_gains(v.stream, d_stats, st.d_offsets.as<long long>(), j.n_canvases, p->sigma_n, p->sigma_g, d_gains, d_status);
    SIFT_HIP_CHECK(hipGetLastError());

    if (!stats_direct) match_download(j.c, j.stats, d_stats, stat_bytes);
    if (want_gains && !gains_direct) match_download(j.c, j.gains, d_gains, gain_bytes);
    if (j.status && want_gains && !status_direct) match_download(j.c, j.status, d_status, (size_t)j.n_canvases);
    match_wait(j.c);
    return SIFT_HIP_OK;
}

}  // namespace
}  // namespace sift_hip

using namespace sift_hip;

extern "C" int sift_hip_overlap_stats(sift_hip_ctx* c, const float* imgs, int n_imgs, int w, int h, int n_canvases, const int64_t* offsets, const int32_t* src,
                                      const float* models, const sift_hip_overlap_params* params, int64_t* stats, float* gains, uint8_t* status, char* err,
                                      int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_overlap_stats: no context (the overlap statistics run on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, imgs, n_imgs, w, h, n_canvases, offsets, src, models, params, stats, gains, status, err, errlen};
    return match_guarded(err, errlen, run, &j);
}
