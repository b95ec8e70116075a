// sift::Matcher — descriptor matching for the points sift::Sift::calculate() returns.  An extension: the reference has no
// matcher, so nothing here mirrors it.  Header-only host code above the C ABI (include/sift_hip.h, "descriptor matching"):
// squared distances on the GPU's f32 matrix cores, the two nearest rows of every query point, ratio test, cross-check.
#ifndef SIFT_AMD_MATCH_HPP
#define SIFT_AMD_MATCH_HPP
#include <algorithm>
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sift_hip.h"
#include "image2f.hpp"
#include "interestpoint.hpp"
#include "types.hpp"

namespace sift {

struct Match {
    int query = -1, train = -1;          // positions in the two lists handed to Matcher::match
    f32_t dist2 = 0.0f, second2 = 0.0f;  // squared distance to the best and to the second best train point (+inf: none)
};

struct Homography {
    f32_t h[9] = {};                     // row-major, query image -> train image: (tx, ty, 1) ~ H (qx, qy, 1); the best minimal-sample model,
                                         // re-estimated over its inliers when Matcher::verify is given refine > 0
    int inliers = 0;
    int iteration = -1;                  // the winning hypothesis; -1: no model (fewer than four matches, or every sample degenerate)
    int refined = 0;                     // refinement rounds accepted, 0 .. refine
    std::vector<unsigned char> inlier;   // one flag per match handed to Matcher::verify
};

struct Fundamental {
    f32_t f[9] = {};                     // row-major, (tx, ty, 1) F (qx, qy, 1)^T = 0 with q in the query and t in the train image: the best
                                         // seven-point model; its entry of largest magnitude is +1
    int inliers = 0;
    int iteration = -1;                  // the winning sample; -1: no model (fewer than seven matches, or every sample degenerate)
    int root = -1;                       // which real root of the winner's cubic, 0 .. 2
    std::vector<unsigned char> inlier;   // one flag per match handed to Matcher::verify_fundamental
};

class Matcher {
public:
    explicit Matcher(int device = 0) {
        char err[512] = "";
        if (sift_hip_create(device, &_ctx, err, sizeof(err)) != SIFT_HIP_OK)
            throw std::runtime_error(std::string("sift_hip_create: ") + err);
    }
    Matcher(const Matcher&) = delete;
    Matcher& operator=(const Matcher&) = delete;
    ~Matcher() { sift_hip_destroy(_ctx); }

    // Matches of `query` among `train`, in the order of `query`.  ratio 0: no ratio test, else 0 < ratio <= 1 (Lowe's test on
    // squared distances: dist2 < ratio^2 * second2); crossCheck: keep a match only if it is also the best one seen from the
    // train point.  A point without a 128-float descriptor takes no part.  quantized: the descriptors are quantised to 8 bits on
    // the GPU and matched by the integer distance on the i8 matrix cores (include/sift_hip.h, "8-bit descriptors and integer
    // matching"); dist2 and second2 are then integers, sum (a - b)^2 over the 128 bytes.
    std::vector<Match> match(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, f32_t ratio = 0.8f,
                             bool crossCheck = false, bool quantized = false) {
        const size_t nq = query.size(), nt = train.size();
        rows(query, train);
        const int64_t offsets[3] = {0, (int64_t)nq, (int64_t)(nq + nt)};
        const int32_t pq = 0, pt = 1;
        sift_hip_match_params prm{};
        prm.ratio = ratio;
        prm.cross_check = crossCheck ? 1 : 0;
        prm.quantized = quantized ? 1 : 0;
        _recs.resize(nq);
        int32_t count = 0;
        int64_t total = 0;
        char err[512] = "";
        const int rc = sift_hip_match(_ctx, _desc.data(), _kp.data(), 2, offsets, 1, &pq, &pt, &prm, _recs.data(), &count, &total, err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        return records((size_t)total);
    }

    // Guided matching (include/sift_hip.h, "guided matching"): match() again under a verified model.  A train point competes for
    // a query point only when it lies within `threshold` pixels of the model - of the transferred point for a Homography, of the
    // epipolar line (Sampson distance) for a Fundamental - so "best" and "second best" are taken among those points alone, and so
    // is the best query point seen from a train point (crossCheck).  Repeated structure, which the plain ratio test drops, comes
    // back.  Coordinates as verify() forms them: loc * 2^octave, halved when the points come from a subpixel run.  A model that
    // is none (iteration -1: all zeros) gives no matches.  Throws std::invalid_argument for a threshold that is not finite and
    // positive and for what match() rejects.  quantized: as for match() - the descriptors are quantised to 8 bits on the GPU and the
    // guided matcher runs on the i8 matrix cores (include/sift_hip.h, "guided matching on 8-bit descriptors").
    std::vector<Match> match_guided(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const Homography& model,
                                    f32_t threshold = 3.0f, f32_t ratio = 0.8f, bool crossCheck = false, bool subpixel = false,
                                    bool quantized = false) {
        return guided(query, train, SIFT_HIP_GUIDE_HOMOGRAPHY, model.h, threshold, ratio, crossCheck, subpixel, quantized);
    }
    std::vector<Match> match_guided(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const Fundamental& model,
                                    f32_t threshold = 3.0f, f32_t ratio = 0.8f, bool crossCheck = false, bool subpixel = false,
                                    bool quantized = false) {
        return guided(query, train, SIFT_HIP_GUIDE_FUNDAMENTAL, model.f, threshold, ratio, crossCheck, subpixel, quantized);
    }

    // The geometric check of a match list (include/sift_hip.h, "geometric verification"): the best four-point homography
    // from the query image to the train image over the matches' image coordinates, loc * 2^octave (halved when the points
    // come from a subpixel run), and one flag per match.  refine: rounds of least-squares re-estimation of the winner over its
    // own inliers, 0 .. 8 (0: the minimal-sample model; the inlier count never decreases).  Throws std::invalid_argument for
    // iterations outside 1 .. 65536, a threshold that is not finite and positive, or refine above 8.
    Homography verify(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const std::vector<Match>& matches,
                      unsigned iterations = 2048, f32_t threshold = 3.0f, unsigned seed = 0, bool subpixel = false, unsigned refine = 0) {
        gather(query, train, matches, subpixel);
        const int64_t offsets[2] = {0, (int64_t)matches.size()};
        sift_hip_ransac_params prm{};
        prm.iterations = iterations;
        prm.seed = seed;
        prm.threshold = threshold;
        prm.refine = refine;
        sift_hip_homography model{};
        Homography out;
        out.inlier.assign(matches.size(), 0);
        char err[512] = "";
        const int rc = sift_hip_ransac_homography(_ctx, _pts.data(), 1, offsets, &prm, &model, out.inlier.data(), nullptr, err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        for (int k = 0; k < 9; ++k) out.h[k] = model.h[k];
        out.inliers = model.inliers;
        out.iteration = model.iteration;
        out.refined = model.refined;
        return out;
    }

    // The epipolar check of a match list (include/sift_hip.h, "epipolar verification"): the best seven-point fundamental matrix
    // over the same coordinates, by the Sampson distance, and one flag per match - for two views of a general scene, where a
    // homography explains the matches of one plane only.  A planar scene or a camera that only rotates does not determine F:
    // verify() is the right call there.  There is no refinement.  Throws std::invalid_argument as verify() does.
    Fundamental verify_fundamental(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const std::vector<Match>& matches,
                                   unsigned iterations = 2048, f32_t threshold = 3.0f, unsigned seed = 0, bool subpixel = false) {
        gather(query, train, matches, subpixel);
        const int64_t offsets[2] = {0, (int64_t)matches.size()};
        sift_hip_ransac_params prm{};
        prm.iterations = iterations;
        prm.seed = seed;
        prm.threshold = threshold;
        sift_hip_fundamental model{};
        Fundamental out;
        out.inlier.assign(matches.size(), 0);
        char err[512] = "";
        const int rc = sift_hip_ransac_fundamental(_ctx, _pts.data(), 1, offsets, &prm, &model, out.inlier.data(), nullptr, err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        for (int k = 0; k < 9; ++k) out.f[k] = model.f[k];
        out.inliers = model.inliers;
        out.iteration = model.iteration;
        out.root = model.root;
        return out;
    }

    // The least-squares refit of a fundamental matrix over its own inliers among `matches` (include/sift_hip.h,
    // sift_hip_refine_fundamental): at most `rounds` rounds, 0 .. 8 (0 only counts), of the normalised eight-point method with a
    // rank-2 step, from `model` as verify_fundamental() returned it.  The inlier count never decreases; a model that is none
    // (iteration -1) comes back as it is.  *refined (may be null): the rounds accepted.  Throws std::invalid_argument for rounds
    // outside 0 .. 8 or a threshold that is not finite and positive.
    Fundamental refine_fundamental(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const std::vector<Match>& matches,
                                   const Fundamental& model, f32_t threshold = 3.0f, int rounds = 2, bool subpixel = false, int* refined = nullptr) {
        gather(query, train, matches, subpixel);
        const int64_t offsets[2] = {0, (int64_t)matches.size()};
        sift_hip_fundamental rec{};
        for (int k = 0; k < 9; ++k) rec.f[k] = model.f[k];
        rec.inliers = model.inliers;
        rec.iteration = model.iteration;
        rec.root = model.root;
        Fundamental out;
        out.inlier.assign(matches.size(), 0);
        int32_t accepted = 0;
        char err[512] = "";
        const int rc = sift_hip_refine_fundamental(_ctx, _pts.data(), 1, offsets, threshold, rounds, &rec, &accepted, out.inlier.data(), err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        for (int k = 0; k < 9; ++k) out.f[k] = rec.f[k];
        out.inliers = rec.inliers;
        out.iteration = rec.iteration;
        out.root = rec.root;
        if (refined) *refined = accepted;
        return out;
    }

    // Sub-pixel coordinates (include/sift_hip.h, "sub-pixel localisation"): from now on verify, verify_fundamental,
    // refine_fundamental and match_guided take a point's image coordinates from these records - what sift::Sift::localize(max_moves)
    // returned after the calculate() of the query list and of the train list, one record per point - instead of loc << octave.  A
    // Matcher holds no pyramid, so the records come from the Sift that made the points.  clear_localize() switches back.
    void localize(std::vector<sift_hip_localized> query, std::vector<sift_hip_localized> train) {
        _loc[0] = std::move(query);
        _loc[1] = std::move(train);
        _use = true;
    }
    void clear_localize() { _use = false; }

    // The homography warp (include/sift_hip.h, "homography warp"): `train` resampled on an out_w x out_h pixel grid of the query
    // frame under the nine floats `h` (verify()'s model maps query to train, so it is taken as it comes); output pixel (x, y) is
    // the query-frame point (x + origin_x, y + origin_y).  Where the train image does not reach: `fill`, and 0 in *covered (may
    // be null; else one byte per pixel).  A model that is none (all zeros) gives an image of `fill`.  Throws
    // std::invalid_argument for what sift_hip_warp_homography rejects.
    Image2f warp(Image2f& train, const f32_t (&h)[9], int out_w, int out_h, int origin_x = 0, int origin_y = 0, f32_t fill = 0.0f,
                 bool bilinear = true, std::vector<uint8_t>* covered = nullptr) {
        sift_hip_warp_params prm{};
        prm.out_w = out_w;
        prm.out_h = out_h;
        prm.origin_x = origin_x;
        prm.origin_y = origin_y;
        prm.fill = fill;
        prm.interp = bilinear ? 1 : 0;
        Image2f out(out_w > 0 ? out_w : 0, out_h > 0 ? out_h : 0);
        if (covered) covered->assign((size_t)out.width() * (size_t)out.height(), 0);
        char err[512] = "";
        const int rc = sift_hip_warp_homography(_ctx, train.data(), 1, (int)train.width(), (int)train.height(), 1, nullptr, h, &prm, out.data(),
                                                covered ? covered->data() : nullptr, nullptr, err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        return out;
    }

    // The compositor (include/sift_hip.h, "compositor"): `frames` (all of one size) accumulated in order on ONE out_w x out_h
    // canvas, frame k under the nine floats models[k] (canvas lattice -> frame, as warp() takes them; the reference frame's is
    // the identity); canvas pixel (x, y) is the lattice point (x + origin_x, y + origin_y).  blend: 0 the first covering
    // frame's value, 1 the mean, 2 feathered by the distance to each frame's border.  Where no frame reaches: `fill`, and 0 in
    // *count (may be null; else the number of covering frames per pixel).  Throws std::invalid_argument for what
    // sift_hip_composite_homography rejects.  gains (may be null; else one per frame, as overlap() returns them): frame k's values
    // are multiplied by (*gains)[k] (sift_hip_composite_homography_gains).
    Image2f composite(const std::vector<Image2f*>& frames, const std::vector<std::array<f32_t, 9>>& models, int out_w, int out_h, int origin_x = 0,
                      int origin_y = 0, int blend = 2, f32_t fill = 0.0f, bool bilinear = true, std::vector<uint16_t>* count = nullptr,
                      const std::vector<f32_t>* gains = nullptr) {
        if (frames.empty() || frames.size() != models.size()) throw std::invalid_argument("composite: one model per frame, at least one frame");
        if (gains && gains->size() != frames.size()) throw std::invalid_argument("composite: one gain per frame");
        const size_t w = frames[0]->width(), h = frames[0]->height();
        std::vector<f32_t> stack(frames.size() * w * h);
        for (size_t k = 0; k < frames.size(); ++k) {
            if (frames[k]->width() != w || frames[k]->height() != h) throw std::invalid_argument("composite: frames of one size");
            std::copy(frames[k]->data(), frames[k]->data() + w * h, stack.begin() + k * w * h);
        }
        sift_hip_composite_params prm{};
        prm.out_w = out_w;
        prm.out_h = out_h;
        prm.origin_x = origin_x;
        prm.origin_y = origin_y;
        prm.fill = fill;
        prm.interp = bilinear ? 1 : 0;
        prm.blend = (uint8_t)blend;
        Image2f out(out_w > 0 ? out_w : 0, out_h > 0 ? out_h : 0);
        if (count) count->assign((size_t)out.width() * (size_t)out.height(), 0);
        const int64_t offsets[2] = {0, (int64_t)frames.size()};
        char err[512] = "";
        const int rc = sift_hip_composite_homography_gains(_ctx, stack.data(), (int)frames.size(), (int)w, (int)h, 1, offsets, nullptr, models[0].data(), &prm,
                                                           gains ? gains->data() : nullptr, out.data(), count ? count->data() : nullptr, nullptr, err,
                                                           sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        return out;
    }

    // The two-band compositor (include/sift_hip.h, "two-band compositor"): composite()'s frames, models, canvas, fill, count and
    // gains, blended in two frequency bands - each frame's low band (a Gaussian blur of `sigma` canvas pixels, normalised by the
    // blur of the frame's coverage) is feathered, its high band is taken from the one covering frame with the largest feather
    // weight, so fine detail is not doubled where the frames overlap.  The taps are the centre-to-edge half of
    // sift_hip_gauss_taps(sigma), whose radius is three sigma and may not exceed 16.  Throws std::invalid_argument for that and
    // for what sift_hip_composite_twoband rejects.
    Image2f composite_twoband(const std::vector<Image2f*>& frames, const std::vector<std::array<f32_t, 9>>& models, int out_w, int out_h, int origin_x = 0,
                              int origin_y = 0, f32_t sigma = 5.0f, f32_t fill = 0.0f, bool bilinear = true, std::vector<uint16_t>* count = nullptr,
                              const std::vector<f32_t>* gains = nullptr) {
        if (frames.empty() || frames.size() != models.size()) throw std::invalid_argument("composite_twoband: one model per frame, at least one frame");
        if (gains && gains->size() != frames.size()) throw std::invalid_argument("composite_twoband: one gain per frame");
        std::vector<f32_t> taps(8192);
        const int radius = sift_hip_gauss_taps(sigma, taps.data(), (int)taps.size());
        if (radius < 0 || radius > 16) throw std::invalid_argument("composite_twoband: sigma must be >= 0 and give a radius (three sigma) of at most 16");
        const size_t w = frames[0]->width(), h = frames[0]->height();
        std::vector<f32_t> stack(frames.size() * w * h);
        for (size_t k = 0; k < frames.size(); ++k) {
            if (frames[k]->width() != w || frames[k]->height() != h) throw std::invalid_argument("composite_twoband: frames of one size");
            std::copy(frames[k]->data(), frames[k]->data() + w * h, stack.begin() + k * w * h);
        }
        sift_hip_twoband_params prm{};
        prm.out_w = out_w;
        prm.out_h = out_h;
        prm.origin_x = origin_x;
        prm.origin_y = origin_y;
        prm.fill = fill;
        prm.interp = bilinear ? 1 : 0;
        prm.radius = (uint8_t)radius;
        Image2f out(out_w > 0 ? out_w : 0, out_h > 0 ? out_h : 0);
        if (count) count->assign((size_t)out.width() * (size_t)out.height(), 0);
        const int64_t offsets[2] = {0, (int64_t)frames.size()};
        char err[512] = "";
        const int rc = sift_hip_composite_twoband(_ctx, stack.data(), (int)frames.size(), (int)w, (int)h, 1, offsets, nullptr, models[0].data(), &prm,
                                                  taps.data() + radius, gains ? gains->data() : nullptr, out.data(), count ? count->data() : nullptr, nullptr,
                                                  err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        return out;
    }

    // The overlap statistics (include/sift_hip.h, "overlap statistics") of `frames` (at most 32, all of one size) placed as for
    // composite(): stats = 4 x 32 x 32 sums over the canvas pixels that frames i and j both cover - N (pixels), S (q_i), SS
    // (q_i^2), X (q_i q_j), q the 8-bit intensity round(value * scale) - and one gain per frame (Brown and Lowe's gain
    // compensation; sigma_n, sigma_g on the 0 .. 255 grid).  solved = false: the solve failed and every gain is 1.
    struct Overlap {
        std::vector<int64_t> stats;
        std::vector<f32_t> gains;
        bool solved;
    };
    Overlap overlap(const std::vector<Image2f*>& frames, const std::vector<std::array<f32_t, 9>>& models, int out_w, int out_h, int origin_x = 0,
                    int origin_y = 0, f32_t scale = 1.0f, bool bilinear = true, f32_t sigma_n = 10.0f, f32_t sigma_g = 0.1f) {
        if (frames.empty() || frames.size() != models.size()) throw std::invalid_argument("overlap: one model per frame, at least one frame");
        const size_t w = frames[0]->width(), h = frames[0]->height();
        std::vector<f32_t> stack(frames.size() * w * h);
        for (size_t k = 0; k < frames.size(); ++k) {
            if (frames[k]->width() != w || frames[k]->height() != h) throw std::invalid_argument("overlap: frames of one size");
            std::copy(frames[k]->data(), frames[k]->data() + w * h, stack.begin() + k * w * h);
        }
        sift_hip_overlap_params prm{};
        prm.out_w = out_w;
        prm.out_h = out_h;
        prm.origin_x = origin_x;
        prm.origin_y = origin_y;
        prm.scale = scale;
        prm.sigma_n = sigma_n;
        prm.sigma_g = sigma_g;
        prm.interp = bilinear ? 1 : 0;
        Overlap r{std::vector<int64_t>(4 * 32 * 32, 0), std::vector<f32_t>(frames.size(), 1.0f), true};
        const int64_t offsets[2] = {0, (int64_t)frames.size()};
        uint8_t status = 0;
        char err[512] = "";
        const int rc = sift_hip_overlap_stats(_ctx, stack.data(), (int)frames.size(), (int)w, (int)h, 1, offsets, nullptr, models[0].data(), &prm,
                                              r.stats.data(), r.gains.data(), &status, err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        r.solved = status == 0;
        return r;
    }

    // The direct alignment (include/sift_hip.h, "direct alignment"): the nine floats `h` (query to train, as verify() returns
    // them) refined IN PLACE on the pixels of the two frames (of one size) by at most `rounds` (0 .. 8) Gauss-Newton steps on
    // sum (query - gain train(H .) - bias)^2; the record says what was reached (h, gain, bias, rms0 -> rms, pixels, rounds,
    // status SIFT_HIP_ALIGN_*).  Throws std::invalid_argument for what sift_hip_align_homography rejects.
    sift_hip_alignment align(Image2f& query, Image2f& train, f32_t (&h)[9], int rounds = 4, int border = 2, int min_pixels = 256,
                             f32_t damping = 0.0f) {
        if (query.width() != train.width() || query.height() != train.height()) throw std::invalid_argument("align: frames of one size");
        const size_t px = (size_t)query.width() * (size_t)query.height();
        std::vector<f32_t> stack(2 * px);
        std::copy(query.data(), query.data() + px, stack.begin());
        std::copy(train.data(), train.data() + px, stack.begin() + px);
        sift_hip_align_params prm{};
        prm.rounds = rounds;
        prm.border = border;
        prm.min_pixels = min_pixels;
        prm.damping = damping;
        sift_hip_homography model{};
        std::copy(h, h + 9, model.h);
        sift_hip_alignment out{};
        const int32_t pq = 0, pt = 1;
        char err[512] = "";
        const int rc = sift_hip_align_homography(_ctx, stack.data(), 2, (int)query.width(), (int)query.height(), 1, &pq, &pt, &prm, &model, &out, nullptr,
                                                 err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        std::copy(model.h, model.h + 9, h);
        return out;
    }

private:
    // the image coordinates of point i of the query (side 0) or train (side 1) list
    void coords(const InterestPoint& p, int side, size_t i, f32_t scale, f32_t* xy) const {
        if (_use) {
            const sift_hip_localized& r = _loc[side].at(i);
            xy[0] = r.x;
            xy[1] = r.y;
        } else {
            xy[0] = (f32_t)((unsigned)p.loc.x << p.octave) * scale;
            xy[1] = (f32_t)((unsigned)p.loc.y << p.octave) * scale;
        }
    }
    // both lists' descriptor rows and valid flags -> _desc, _kp
    void rows(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train) {
        const size_t nq = query.size(), nt = train.size();
        _desc.assign((nq + nt) * 128, 0.0f);
        _kp.assign(nq + nt, sift_hip_keypoint{});
        for (size_t i = 0; i < nq + nt; ++i) {
            const InterestPoint& p = i < nq ? query[i] : train[i - nq];
            if (p.descriptors.size() != 128) continue;
            _kp[i].has_descriptor = 1;
            for (size_t k = 0; k < 128; ++k) _desc[i * 128 + k] = p.descriptors[k];
        }
    }
    std::vector<Match> records(size_t total) const {
        std::vector<Match> out(total);
        for (size_t i = 0; i < out.size(); ++i) {
            out[i].query = _recs[i].query;
            out[i].train = _recs[i].train;
            out[i].dist2 = _recs[i].dist2;
            out[i].second2 = _recs[i].second2;
        }
        return out;
    }
    std::vector<Match> guided(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, unsigned kind, const f32_t (&m)[9],
                              f32_t threshold, f32_t ratio, bool crossCheck, bool subpixel, bool quantized) {
        const size_t nq = query.size(), nt = train.size();
        rows(query, train);
        const f32_t scale = subpixel ? 0.5f : 1.0f;
        _xy.resize((nq + nt) * 2);
        for (size_t i = 0; i < nq + nt; ++i) {   // every point's image coordinates, as gather() forms them per match
            coords(i < nq ? query[i] : train[i - nq], i < nq ? 0 : 1, i < nq ? i : i - nq, scale, &_xy[2 * i]);
        }
        const int64_t offsets[3] = {0, (int64_t)nq, (int64_t)(nq + nt)};
        const int32_t pq = 0, pt = 1;
        sift_hip_match_params prm{};
        prm.ratio = ratio;
        prm.cross_check = crossCheck ? 1 : 0;
        sift_hip_guide_params guide{};
        guide.model = kind;
        guide.threshold = threshold;
        _recs.resize(nq);
        int32_t count = 0;
        int64_t total = 0;
        char err[512] = "";
        int rc;
        if (quantized) {   // the bytes of sift_hip_quantize through the byte call
            _desc8.resize(_desc.size());
            rc = sift_hip_quantize(_ctx, _desc.data(), (int64_t)(nq + nt), _desc8.data(), err, sizeof(err));
            if (rc == SIFT_HIP_OK)
                rc = sift_hip_match_guided_u8(_ctx, _desc8.data(), _kp.data(), _xy.data(), 2, offsets, 1, &pq, &pt, &prm, &guide, m, _recs.data(),
                                              &count, &total, err, sizeof(err));
        } else {
            rc = sift_hip_match_guided(_ctx, _desc.data(), _kp.data(), _xy.data(), 2, offsets, 1, &pq, &pt, &prm, &guide, m, _recs.data(), &count,
                                       &total, err, sizeof(err));
        }
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        return records((size_t)total);
    }
    // the matches' image coordinates -> _pts, rows (qx, qy, tx, ty)
    void gather(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const std::vector<Match>& matches, bool subpixel) {
        const f32_t scale = subpixel ? 0.5f : 1.0f;
        _pts.resize(matches.size() * 4);
        for (size_t i = 0; i < matches.size(); ++i) {
            coords(query.at((size_t)matches[i].query), 0, (size_t)matches[i].query, scale, &_pts[4 * i]);
            coords(train.at((size_t)matches[i].train), 1, (size_t)matches[i].train, scale, &_pts[4 * i + 2]);
        }
    }


    sift_hip_ctx* _ctx = nullptr;
    std::vector<float> _desc;              // both lists' rows back to back, kept between calls
    std::vector<uint8_t> _desc8;           // guided matching with quantized: the rows as bytes
    std::vector<sift_hip_keypoint> _kp;
    std::vector<sift_hip_match_rec> _recs;
    std::vector<float> _pts;
    std::vector<float> _xy;                // guided matching: both lists' image coordinates
    std::vector<sift_hip_localized> _loc[2];   // localize(): the query and the train list's records
    bool _use = false;
};

}  // namespace sift
#endif
