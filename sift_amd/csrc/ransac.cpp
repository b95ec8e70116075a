// Host side of the geometric verification (include/sift_hip.h: sift_hip_ransac_homography, sift_hip_result_verify, and their
// fundamental-matrix counterparts sift_hip_ransac_fundamental, sift_hip_result_verify_fundamental): staging of
// caller memory, the tile table that makes all sets one launch of the scoring kernel, and the scratch memory, which the first call
// of a context allocates and the context keeps - outside the batch arena, like the matcher's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "ransac_kernels.h"

namespace sift_hip {

struct RansacState {
    ScratchBuf d_pts;                        // rows that arrive in host memory, or that sift_hip_result_verify builds
    ScratchBuf d_off, d_tiles, d_kp_row0;    // the tables
    ScratchBuf d_hyp, d_scores;              // every hypothesis' model and score
    ScratchBuf d_models, d_inlier;           // results on their way to host memory
    void* h_tables = nullptr;                // page-locked image of the tables (the copies are asynchronous)
    size_t h_cap = 0;
};

void ransac_state_free(RansacState* st) {
    if (!st) return;
    for (ScratchBuf* b : {&st->d_pts, &st->d_off, &st->d_tiles, &st->d_kp_row0, &st->d_hyp, &st->d_scores, &st->d_models, &st->d_inlier}) b->release();
    if (st->h_tables) {
        ApiGuard api;
        (void)hipHostFree(st->h_tables);
    }
    delete st;
}

namespace {

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

int fail(char* err, int errlen, const char* msg) {
    match_set_err(err, errlen, msg);
    return SIFT_HIP_EINVAL;
}

int check_params(const sift_hip_ransac_params* p, char* err, int errlen) {
    if (!p) return fail(err, errlen, "sift_hip ransac: no parameters");
    if (p->iterations < 1 || p->iterations > 65536) return fail(err, errlen, "sift_hip ransac: iterations must be 1 .. 65536");
    if (!(std::isfinite(p->threshold) && p->threshold > 0.0f)) return fail(err, errlen, "sift_hip ransac: threshold must be finite and > 0");
    if (p->refine > 8) return fail(err, errlen, "sift_hip ransac: refine must be 0 .. 8");
    return SIFT_HIP_OK;
}

// What both entries share.  `pts`: the caller's rows (host or device memory), or null when `gather` builds them from the
// matcher's device-side list.
struct Gather {
    const sift_hip_match_rec* d_recs;
    const sift_hip_keypoint* d_kp;
    const int* kp_row0;   // host: 2 ints per pair
    float coord_scale;
};
struct Job {
    sift_hip_ctx* c;
    const float* pts;
    const Gather* gather;
    int n_sets;
    const int64_t* offsets;
    const sift_hip_ransac_params* params;
    void* models;               // sift_hip_homography, or sift_hip_fundamental when `fund`: records of one size
    uint8_t* inlier;
    int32_t* scores;
    char* err;
    int errlen;
    bool refine_only = false;   // sift_hip_refine_homography: `models` are the caller's, no sampling; params is null
    float threshold = 0.0f;     //   its threshold and rounds
    int rounds = 0;
    bool fund = false;          // the fundamental matrix: seven-point samples, three hypothesis slots per sample, no refinement
};

int run(void* arg) {
    const Job& j = *static_cast<const Job*>(arg);
    const MatchCtxView v = match_ctx_view(j.c);
    SIFT_HIP_CHECK(hipSetDevice(v.device));

    // ---- arguments ----
    if (j.refine_only) {
        if (!(std::isfinite(j.threshold) && j.threshold > 0.0f)) return fail(j.err, j.errlen, "sift_hip ransac: threshold must be finite and > 0");
        if (j.rounds < 0 || j.rounds > 8) return fail(j.err, j.errlen, "sift_hip ransac: rounds must be 0 .. 8");
    } else if (const int rc = check_params(j.params, j.err, j.errlen)) {
        return rc;
    } else if (j.fund && j.params->refine != 0) {
        return fail(j.err, j.errlen, "sift_hip ransac: refine must be 0 for the fundamental matrix (no least-squares refit of F)");
    }
    if (j.n_sets < 0 || (j.n_sets > 0 && (!j.offsets || !j.models))) return fail(j.err, j.errlen, "sift_hip ransac: bad set arguments");
    if (j.n_sets == 0) return SIFT_HIP_OK;
    if (j.offsets[0] < 0) return fail(j.err, j.errlen, "sift_hip ransac: offsets must start at >= 0");
    for (int s = 0; s < j.n_sets; ++s)
        if (j.offsets[s + 1] < j.offsets[s]) return fail(j.err, j.errlen, "sift_hip ransac: offsets must ascend");
    const long long rows = (long long)j.offsets[j.n_sets];
    if (rows > 0x7fffffffLL / 4) return fail(j.err, j.errlen, "sift_hip ransac: too many rows");
    if (rows > 0 && !j.pts && !j.gather) return fail(j.err, j.errlen, "sift_hip ransac: no rows");
    const uint32_t iters = j.refine_only ? 0u : j.params->iterations;
    const uint32_t slots = iters * (j.fund ? 3u : 1u);   // hypotheses per set
    const long long min_rows = j.fund ? kFundMinRows : kHomographyMinRows;
    const long long n_hyp = (long long)j.n_sets * slots;
    if (n_hyp > 0x7fffffffLL / 2) return fail(j.err, j.errlen, "sift_hip ransac: too many hypotheses (sets x iterations)");
    const float thr = j.refine_only ? j.threshold : j.params->threshold, thr2 = thr * thr;
    const int rounds = j.refine_only ? j.rounds : (int)j.params->refine;

    // ---- the tile table: every set's hypothesis blocks against every range of its rows ----
    std::vector<RansacTile> tiles;
    long long n_tiles = 0;
    for (int s = 0; s < j.n_sets; ++s) {
        const long long m = j.offsets[s + 1] - j.offsets[s];
        if (m >= min_rows && !j.refine_only) n_tiles += ((slots + kRansacHyps - 1) / kRansacHyps) * ((m + kRansacRows - 1) / kRansacRows);
    }
    if (n_tiles > 0x7fffffffLL / 16) return fail(j.err, j.errlen, "sift_hip ransac: too many tiles");
    tiles.reserve((size_t)n_tiles);
    for (int s = 0; s < j.n_sets; ++s) {
        const long long r0 = j.offsets[s], m = j.offsets[s + 1] - r0;
        if (m < min_rows || j.refine_only) continue;   // no hypothesis of such a set is valid
        for (long long lo = 0; lo < m; lo += kRansacRows)
            for (uint32_t h0 = 0; h0 < slots; h0 += kRansacHyps)
                tiles.push_back(RansacTile{s, (int)h0, (int)(r0 + lo), (int)(r0 + std::min<long long>(m, lo + kRansacRows))});
    }

    RansacState** slot = ransac_ctx_state(j.c);
    if (!*slot) *slot = new RansacState();
    RansacState& st = **slot;

    // ---- rows on the device ----
    const float* d_pts = j.pts;
    if (j.gather || (rows > 0 && !match_ptr_on_device(j.pts))) {
        st.d_pts.ensure((size_t)std::max<long long>(rows, 1) * 4 * sizeof(float));
        if (!j.gather) {
            match_upload(j.c, st.d_pts.p, j.pts, (size_t)rows * 4 * sizeof(float));
            match_wait(j.c);   // pageable memory travels through the context's two staging buffers: the next upload refills them
        }
        d_pts = st.d_pts.as<float>();
    } else if (rows > 0 && (reinterpret_cast<uintptr_t>(j.pts) & 15u) != 0) {
        return fail(j.err, j.errlen, "sift_hip ransac: rows in device memory must be 16-byte aligned");
    }

    // ---- the tables ----
    const size_t b_off = align256(((size_t)j.n_sets + 1) * sizeof(int64_t)), b_tiles = align256(tiles.size() * sizeof(RansacTile)),
                 b_row0 = align256(j.gather ? (size_t)j.n_sets * 2 * sizeof(int) : 0);
    if (b_off + b_tiles + b_row0 > st.h_cap) {
        ApiGuard api;
        if (st.h_tables) SIFT_HIP_CHECK(hipHostFree(st.h_tables));
        st.h_tables = nullptr;
        st.h_cap = 0;
        SIFT_HIP_CHECK(hipHostMalloc(&st.h_tables, 2 * (b_off + b_tiles + b_row0), hipHostMallocDefault));
        st.h_cap = 2 * (b_off + b_tiles + b_row0);
    }
    char* h = static_cast<char*>(st.h_tables);
    std::memcpy(h, j.offsets, ((size_t)j.n_sets + 1) * sizeof(int64_t));
    std::memcpy(h + b_off, tiles.data(), tiles.size() * sizeof(RansacTile));
    if (j.gather) std::memcpy(h + b_off + b_tiles, j.gather->kp_row0, (size_t)j.n_sets * 2 * sizeof(int));
    st.d_off.ensure(b_off);
    st.d_tiles.ensure(std::max<size_t>(b_tiles, 256));
    SIFT_HIP_CHECK(hipMemcpyAsync(st.d_off.p, h, b_off, hipMemcpyHostToDevice, v.stream));
    if (!tiles.empty()) SIFT_HIP_CHECK(hipMemcpyAsync(st.d_tiles.p, h + b_off, b_tiles, hipMemcpyHostToDevice, v.stream));
    if (j.gather) {
        st.d_kp_row0.ensure(b_row0);
        SIFT_HIP_CHECK(hipMemcpyAsync(st.d_kp_row0.p, h + b_off + b_tiles, b_row0, hipMemcpyHostToDevice, v.stream));
    }

    // ---- results: written in place when the caller's array is device memory ----
    const bool models_direct = match_ptr_on_device(j.models), inlier_direct = j.inlier && match_ptr_on_device(j.inlier),
               scores_direct = j.scores && match_ptr_on_device(j.scores);
    st.d_hyp.ensure((size_t)std::max<long long>(n_hyp, 1) * sizeof(RansacHyp));
    if (!scores_direct) st.d_scores.ensure((size_t)std::max<long long>(n_hyp, 1) * sizeof(int32_t));
    if (!models_direct) st.d_models.ensure((size_t)j.n_sets * sizeof(sift_hip_homography));
    if (j.inlier && !inlier_direct) st.d_inlier.ensure((size_t)std::max<long long>(rows, 1));
    int32_t* d_scores = scores_direct ? j.scores : st.d_scores.as<int32_t>();
    void* d_models = models_direct ? j.models : st.d_models.p;
    sift_hip_homography* d_hmodels = static_cast<sift_hip_homography*>(d_models);
    sift_hip_fundamental* d_fmodels = static_cast<sift_hip_fundamental*>(d_models);
    uint8_t* d_inlier = inlier_direct ? j.inlier : st.d_inlier.as<uint8_t>();

    // ---- the launches: one of each kernel, whatever the number of sets ----
    if (j.gather)
        launch_ransac_gather(v.stream, j.gather->d_recs, st.d_off.as<int64_t>(), j.n_sets, rows, j.gather->d_kp, st.d_kp_row0.as<int>(),
                             j.gather->coord_scale, st.d_pts.as<float>());
    if (j.refine_only) {
        if (!models_direct) {
            match_upload(j.c, d_models, j.models, (size_t)j.n_sets * sizeof(sift_hip_homography));
            match_wait(j.c);
        }
    } else if (j.fund) {
        SIFT_HIP_CHECK(hipMemsetAsync(d_scores, 0, (size_t)n_hyp * sizeof(int32_t), v.stream));
        launch_fund_hypotheses(v.stream, d_pts, st.d_off.as<int64_t>(), j.n_sets, iters, j.params->seed, st.d_hyp.as<RansacHyp>());
        launch_fund_score(v.stream, d_pts, st.d_hyp.as<RansacHyp>(), st.d_tiles.as<RansacTile>(), (int)tiles.size(), slots, thr2, d_scores);
        launch_fund_select(v.stream, st.d_hyp.as<RansacHyp>(), j.n_sets, slots, d_scores, d_fmodels);
    } else {
        SIFT_HIP_CHECK(hipMemsetAsync(d_scores, 0, (size_t)n_hyp * sizeof(int32_t), v.stream));
        launch_ransac_hypotheses(v.stream, d_pts, st.d_off.as<int64_t>(), j.n_sets, iters, j.params->seed, st.d_hyp.as<RansacHyp>());
        launch_ransac_score(v.stream, d_pts, st.d_hyp.as<RansacHyp>(), st.d_tiles.as<RansacTile>(), (int)tiles.size(), iters, thr2, d_scores);
        launch_ransac_select(v.stream, st.d_hyp.as<RansacHyp>(), j.n_sets, iters, d_scores, d_hmodels);
    }
    // every round of every set in one launch; with refine 0 the models are the selection's
    if (j.refine_only || rounds > 0) launch_ransac_refine(v.stream, d_pts, st.d_off.as<int64_t>(), j.n_sets, rounds, thr2, d_hmodels);
    if (j.inlier && j.fund) launch_fund_flags(v.stream, d_pts, st.d_off.as<int64_t>(), j.n_sets, rows, d_fmodels, thr2, d_inlier);
    if (j.inlier && !j.fund) launch_ransac_flags(v.stream, d_pts, st.d_off.as<int64_t>(), j.n_sets, rows, d_hmodels, thr2, d_inlier);
    SIFT_HIP_CHECK(hipGetLastError());

    if (!models_direct) match_download(j.c, j.models, d_models, (size_t)j.n_sets * sizeof(sift_hip_homography));
    if (j.inlier && !inlier_direct) match_download(j.c, j.inlier, d_inlier, (size_t)rows);
    if (j.scores && !scores_direct) match_download(j.c, j.scores, d_scores, (size_t)n_hyp * sizeof(int32_t));
    match_wait(j.c);
    return SIFT_HIP_OK;
}

}  // namespace
}  // namespace sift_hip

using namespace sift_hip;

extern "C" {

int sift_hip_ransac_homography(sift_hip_ctx* c, const float* pts, int n_sets, const int64_t* offsets, const sift_hip_ransac_params* params,
                               sift_hip_homography* models, uint8_t* inlier, int32_t* scores, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_ransac_homography: no context (the verification runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, pts, nullptr, n_sets, offsets, params, models, inlier, scores, err, errlen};
    return match_guarded(err, errlen, run, &j);
}

int sift_hip_refine_homography(sift_hip_ctx* c, const float* pts, int n_sets, const int64_t* offsets, float threshold, int rounds,
                               sift_hip_homography* models, uint8_t* inlier, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_refine_homography: no context (the refinement runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, pts, nullptr, n_sets, offsets, nullptr, models, inlier, nullptr, err, errlen};
    j.refine_only = true;
    j.threshold = threshold;
    j.rounds = rounds;
    return match_guarded(err, errlen, run, &j);
}

}  // extern "C"

// sift_hip_result_verify and sift_hip_result_verify_fundamental: the match, then the model over the gathered coordinates
static int result_verify(bool fund, sift_hip_ctx* c, int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* match_params,
                         const sift_hip_ransac_params* ransac_params, sift_hip_match_rec* recs, int32_t* counts, int64_t* total, void* models,
                         uint8_t* inlier, char* err, int errlen) {
    const char* who = fund ? "sift_hip_result_verify_fundamental" : "sift_hip_result_verify";
    const auto bad = [&](const char* what) {
        match_set_err(err, errlen, (std::string(who) + ": " + what).c_str());
        return SIFT_HIP_EINVAL;
    };
    if (!c) return bad("no context (the verification runs on the GPU only)");
    if (!match_params) return bad("no match parameters");
    if (const int rc = check_params(ransac_params, err, errlen)) return rc;
    if (fund && ransac_params->refine != 0) return fail(err, errlen, "sift_hip ransac: refine must be 0 for the fundamental matrix (no least-squares refit of F)");
    if (n_pairs > 0 && !models) return bad("no model array");
    std::vector<int32_t> host_counts((size_t)std::max(n_pairs, 0), 0);
    const sift_hip_match_rec* d_recs = nullptr;
    const int rc = match_result_on_device(c, who, n_pairs, pair_q, pair_t, match_params, recs, counts, total, &d_recs,
                                          host_counts.data(), err, errlen);
    if (rc != SIFT_HIP_OK || n_pairs <= 0) return rc;
    // pair p is set p: its rows are its records; the keypoints of a record are rows of the pair's two images
    const MatchCtxView v = match_ctx_view(c);
    std::vector<int> img_row0((size_t)v.n_images + 1, 0);
    for (int i = 0; i < v.n_images; ++i) img_row0[(size_t)i + 1] = img_row0[(size_t)i] + v.counts[i];
    std::vector<int64_t> offsets((size_t)n_pairs + 1, 0);
    std::vector<int> kp_row0((size_t)n_pairs * 2, 0);
    for (int p = 0; p < n_pairs; ++p) {
        offsets[(size_t)p + 1] = offsets[(size_t)p] + host_counts[(size_t)p];
        kp_row0[2 * (size_t)p] = img_row0[(size_t)pair_q[p]];       // the indices passed the matcher's check
        kp_row0[2 * (size_t)p + 1] = img_row0[(size_t)pair_t[p]];
    }
    const Gather g{d_recs, v.d_kp, kp_row0.data(), ransac_ctx_subpixel(c) ? 0.5f : 1.0f};
    Job j{c, nullptr, &g, n_pairs, offsets.data(), ransac_params, models, inlier, nullptr, err, errlen};
    j.fund = fund;
    return match_guarded(err, errlen, run, &j);
}

extern "C" {

int sift_hip_result_verify(sift_hip_ctx* c, int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* match_params,
                           const sift_hip_ransac_params* ransac_params, sift_hip_match_rec* recs, int32_t* counts, int64_t* total,
                           sift_hip_homography* models, uint8_t* inlier, char* err, int errlen) {
    return result_verify(false, c, n_pairs, pair_q, pair_t, match_params, ransac_params, recs, counts, total, models, inlier, err, errlen);
}

int sift_hip_ransac_fundamental(sift_hip_ctx* c, const float* pts, int n_sets, const int64_t* offsets, const sift_hip_ransac_params* params,
                                sift_hip_fundamental* models, uint8_t* inlier, int32_t* scores, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_ransac_fundamental: no context (the verification runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, pts, nullptr, n_sets, offsets, params, models, inlier, scores, err, errlen};
    j.fund = true;
    return match_guarded(err, errlen, run, &j);
}

int sift_hip_result_verify_fundamental(sift_hip_ctx* c, int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* match_params,
                                       const sift_hip_ransac_params* ransac_params, sift_hip_match_rec* recs, int32_t* counts, int64_t* total,
                                       sift_hip_fundamental* models, uint8_t* inlier, char* err, int errlen) {
    return result_verify(true, c, n_pairs, pair_q, pair_t, match_params, ransac_params, recs, counts, total, models, inlier, err, errlen);
}

}  // extern "C"
