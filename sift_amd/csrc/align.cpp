// Host side of the direct alignment (include/sift_hip.h: sift_hip_align_homography): checks, staging of caller memory, the
// scratch memory, which the first call of a context allocates and the context keeps, and the passes: rounds + 1 times the
// accumulate and the solve launch on the context's stream, with no synchronisation in between - a pair that has stopped says so
// in its device record.  The kernels: kernels_align.hip; the definition: align_math.h.
#include <cstring>
#include <string>

#include "align_kernels.h"
#include "common.h"

namespace sift_hip {

struct AlignScratch {
    ScratchBuf d_imgs, d_models, d_pairs;        // what arrives in host memory
    ScratchBuf d_out, d_sums;                    // results on their way to host memory
    ScratchBuf d_state, d_partials;              // the pairs' records and the tiles' sums
};

void align_state_free(AlignScratch* st) {
    if (!st) return;
    for (ScratchBuf* b : {&st->d_imgs, &st->d_models, &st->d_pairs, &st->d_out, &st->d_sums, &st->d_state, &st->d_partials}) b->release();
    delete st;
}

namespace {

struct Job {
    sift_hip_ctx* c;
    const float* imgs;
    int n_imgs, w, h, n_pairs;
    const int32_t *pair_q, *pair_t;
    const sift_hip_align_params* p;
    sift_hip_homography* models;
    sift_hip_alignment* out;
    double* sums;
    char* err;
    int errlen;
};

int fail(const Job& j, const char* msg) {
    match_set_err(j.err, j.errlen, (std::string("sift_hip_align_homography: ") + msg).c_str());
    return SIFT_HIP_EINVAL;
}

int run(void* arg) {
    const Job& j = *static_cast<const Job*>(arg);
    const sift_hip_align_params* p = j.p;
    if (!p) return fail(j, "no parameters");
    if (j.n_imgs < 1 || j.w < 1 || j.h < 1 || j.w > kWarpMaxSide || j.h > kWarpMaxSide) return fail(j, "images are n_imgs >= 1 of 1 .. 2^22 pixels a side");
    if (j.n_pairs < 0 || j.n_pairs > 65535) return fail(j, "n_pairs must be 0 .. 65535");
    if (p->rounds < 0 || p->rounds > kAlignMaxRounds) return fail(j, "rounds must be 0 .. 8");
    if (!(p->damping >= 0.0f) || p->damping - p->damping != 0.0f) return fail(j, "damping must be finite and >= 0");
    if (p->border < 0 || 2 * (long long)p->border >= (j.w < j.h ? j.w : j.h)) return fail(j, "border must be >= 0 and below half of either side");
    if (p->path > 1) return fail(j, "path must be 0 or 1");
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return fail(j, "the reserved bytes must be zero");
    if (j.n_pairs == 0) return SIFT_HIP_OK;
    if (!j.imgs || !j.pair_q || !j.pair_t || !j.models || !j.out) return fail(j, "a null argument");
    for (int k = 0; k < j.n_pairs; ++k)
        if (j.pair_q[k] < 0 || j.pair_q[k] >= j.n_imgs || j.pair_t[k] < 0 || j.pair_t[k] >= j.n_imgs) return fail(j, "a pair index outside the images");
    const long long tiles_x = (j.w + kAlignTile - 1) / kAlignTile, tiles_y = (j.h + kAlignTile - 1) / kAlignTile;
    if (tiles_x * tiles_y > 0x7fffffffll / kAlignRec) return fail(j, "the frame has too many tiles");

    const MatchCtxView v = match_ctx_view(j.c);
    SIFT_HIP_CHECK(hipSetDevice(v.device));
    AlignScratch** slot = align_ctx_state(j.c);
    if (!*slot) *slot = new AlignScratch();
    AlignScratch& st = **slot;

    // ---- inputs on the device ----
    const size_t img_bytes = (size_t)j.n_imgs * (size_t)j.w * (size_t)j.h * sizeof(float), model_bytes = (size_t)j.n_pairs * sizeof(sift_hip_homography);
    const float* d_imgs = j.imgs;
    if (!match_ptr_on_device(j.imgs)) {
        st.d_imgs.ensure(img_bytes);
        match_upload(j.c, st.d_imgs.p, j.imgs, img_bytes);
        match_wait(j.c);   // pageable memory travels through the context's two staging buffers: the next upload refills them
        d_imgs = st.d_imgs.as<float>();
    }
    const bool models_direct = match_ptr_on_device(j.models), out_direct = match_ptr_on_device(j.out);
    sift_hip_homography* d_models = j.models;
    if (!models_direct) {
        st.d_models.ensure(model_bytes);
        match_upload(j.c, st.d_models.p, j.models, model_bytes);
        match_wait(j.c);
        d_models = st.d_models.as<sift_hip_homography>();
    }
    const size_t pair_bytes = (size_t)j.n_pairs * sizeof(int);
    st.d_pairs.ensure(2 * pair_bytes);
    match_upload(j.c, st.d_pairs.p, j.pair_q, pair_bytes);
    match_wait(j.c);
    match_upload(j.c, st.d_pairs.as<char>() + pair_bytes, j.pair_t, pair_bytes);
    match_wait(j.c);
    const int* d_pair_q = st.d_pairs.as<int>();
    const int* d_pair_t = d_pair_q + j.n_pairs;

    // ---- results and scratch ----
    const size_t out_bytes = (size_t)j.n_pairs * sizeof(sift_hip_alignment), sum_bytes = (size_t)j.n_pairs * kAlignRec * sizeof(double);
    if (!out_direct) st.d_out.ensure(out_bytes);
    sift_hip_alignment* d_out = out_direct ? j.out : st.d_out.as<sift_hip_alignment>();
    st.d_sums.ensure(sum_bytes);
    st.d_state.ensure((size_t)j.n_pairs * sizeof(AlignState));
    st.d_partials.ensure((size_t)j.n_pairs * (size_t)(tiles_x * tiles_y) * kAlignRec * sizeof(double));

    const AlignArgs a{j.w, j.h, j.n_pairs, (int)tiles_x, (int)tiles_y, p->rounds, p->border, p->min_pixels, (int)p->path, p->damping, align_norm(j.w, j.h)};
    launch_align_begin(v.stream, d_models, j.n_pairs, st.d_state.as<AlignState>(), d_out, st.d_sums.as<double>());
    for (int k = 0; k <= p->rounds; ++k) {
        launch_align_accumulate(v.stream, d_imgs, d_pair_q, d_pair_t, st.d_state.as<AlignState>(), a, st.d_partials.as<double>());
        launch_align_solve(v.stream, st.d_partials.as<double>(), a, k, st.d_state.as<AlignState>(), d_models, d_out, st.d_sums.as<double>());
    }
    SIFT_HIP_CHECK(hipGetLastError());

    if (!models_direct) match_download(j.c, j.models, d_models, model_bytes);
    if (!out_direct) match_download(j.c, j.out, d_out, out_bytes);
    if (j.sums) match_download(j.c, j.sums, st.d_sums.p, sum_bytes);
    match_wait(j.c);
    return SIFT_HIP_OK;
}

}  // namespace
}  // namespace sift_hip

using namespace sift_hip;

extern "C" int sift_hip_align_homography(sift_hip_ctx* c, const float* imgs, int n_imgs, int w, int h, int n_pairs, const int32_t* pair_q,
                                         const int32_t* pair_t, const sift_hip_align_params* params, sift_hip_homography* models, sift_hip_alignment* out,
                                         double* sums, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_align_homography: no context (the alignment runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, imgs, n_imgs, w, h, n_pairs, pair_q, pair_t, params, models, out, sums, err, errlen};
    return match_guarded(err, errlen, run, &j);
}
