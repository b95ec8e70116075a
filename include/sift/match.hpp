// sift::Matcher — descriptor matching for the points sift::Sift::calculate() returns.  An extension: the reference has no
// matcher, so nothing here mirrors it.  Header-only host code above the C ABI (include/sift_hip.h, "descriptor matching"):
// squared distances on the GPU's f32 matrix cores, the two nearest rows of every query point, ratio test, cross-check.
#ifndef SIFT_AMD_MATCH_HPP
#define SIFT_AMD_MATCH_HPP
#include <stdexcept>
#include <string>
#include <vector>

#include "../sift_hip.h"
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
    // positive and for what match() rejects.
    std::vector<Match> match_guided(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const Homography& model,
                                    f32_t threshold = 3.0f, f32_t ratio = 0.8f, bool crossCheck = false, bool subpixel = false) {
        return guided(query, train, SIFT_HIP_GUIDE_HOMOGRAPHY, model.h, threshold, ratio, crossCheck, subpixel);
    }
    std::vector<Match> match_guided(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const Fundamental& model,
                                    f32_t threshold = 3.0f, f32_t ratio = 0.8f, bool crossCheck = false, bool subpixel = false) {
        return guided(query, train, SIFT_HIP_GUIDE_FUNDAMENTAL, model.f, threshold, ratio, crossCheck, subpixel);
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

private:
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
                              f32_t threshold, f32_t ratio, bool crossCheck, bool subpixel) {
        const size_t nq = query.size(), nt = train.size();
        rows(query, train);
        const f32_t scale = subpixel ? 0.5f : 1.0f;
        _xy.resize((nq + nt) * 2);
        for (size_t i = 0; i < nq + nt; ++i) {   // every point's image coordinates, as gather() forms them per match
            const InterestPoint& p = i < nq ? query[i] : train[i - nq];
            _xy[2 * i] = (f32_t)((unsigned)p.loc.x << p.octave) * scale;
            _xy[2 * i + 1] = (f32_t)((unsigned)p.loc.y << p.octave) * scale;
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
        const int rc = sift_hip_match_guided(_ctx, _desc.data(), _kp.data(), _xy.data(), 2, offsets, 1, &pq, &pt, &prm, &guide, m, _recs.data(), &count,
                                             &total, err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        return records((size_t)total);
    }
    // the matches' image coordinates -> _pts, rows (qx, qy, tx, ty)
    void gather(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, const std::vector<Match>& matches, bool subpixel) {
        const f32_t scale = subpixel ? 0.5f : 1.0f;
        _pts.resize(matches.size() * 4);
        for (size_t i = 0; i < matches.size(); ++i) {
            const InterestPoint& q = query.at((size_t)matches[i].query);
            const InterestPoint& t = train.at((size_t)matches[i].train);
            _pts[4 * i] = (f32_t)((unsigned)q.loc.x << q.octave) * scale;
            _pts[4 * i + 1] = (f32_t)((unsigned)q.loc.y << q.octave) * scale;
            _pts[4 * i + 2] = (f32_t)((unsigned)t.loc.x << t.octave) * scale;
            _pts[4 * i + 3] = (f32_t)((unsigned)t.loc.y << t.octave) * scale;
        }
    }


    sift_hip_ctx* _ctx = nullptr;
    std::vector<float> _desc;              // both lists' rows back to back, kept between calls
    std::vector<sift_hip_keypoint> _kp;
    std::vector<sift_hip_match_rec> _recs;
    std::vector<float> _pts;
    std::vector<float> _xy;                // guided matching: both lists' image coordinates
};

}  // namespace sift
#endif
