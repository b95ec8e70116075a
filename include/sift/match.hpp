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
    // train point.  A point without a 128-float descriptor takes no part.
    std::vector<Match> match(const std::vector<InterestPoint>& query, const std::vector<InterestPoint>& train, f32_t ratio = 0.8f,
                             bool crossCheck = false) {
        const size_t nq = query.size(), nt = train.size();
        _desc.assign((nq + nt) * 128, 0.0f);
        _kp.assign(nq + nt, sift_hip_keypoint{});
        for (size_t i = 0; i < nq + nt; ++i) {
            const InterestPoint& p = i < nq ? query[i] : train[i - nq];
            if (p.descriptors.size() != 128) continue;
            _kp[i].has_descriptor = 1;
            for (size_t k = 0; k < 128; ++k) _desc[i * 128 + k] = p.descriptors[k];
        }
        const int64_t offsets[3] = {0, (int64_t)nq, (int64_t)(nq + nt)};
        const int32_t pq = 0, pt = 1;
        sift_hip_match_params prm{};
        prm.ratio = ratio;
        prm.cross_check = crossCheck ? 1 : 0;
        _recs.resize(nq);
        int32_t count = 0;
        int64_t total = 0;
        char err[512] = "";
        const int rc = sift_hip_match(_ctx, _desc.data(), _kp.data(), 2, offsets, 1, &pq, &pt, &prm, _recs.data(), &count, &total, err, sizeof(err));
        if (rc == SIFT_HIP_EINVAL) throw std::invalid_argument(err);
        if (rc != SIFT_HIP_OK) throw std::runtime_error(err);
        std::vector<Match> out((size_t)total);
        for (size_t i = 0; i < out.size(); ++i) {
            out[i].query = _recs[i].query;
            out[i].train = _recs[i].train;
            out[i].dist2 = _recs[i].dist2;
            out[i].second2 = _recs[i].second2;
        }
        return out;
    }

private:
    sift_hip_ctx* _ctx = nullptr;
    std::vector<float> _desc;              // both lists' rows back to back, kept between calls
    std::vector<sift_hip_keypoint> _kp;
    std::vector<sift_hip_match_rec> _recs;
};

}  // namespace sift
#endif
