// Two images -> matches.txt and inliers.txt: sift::Sift::calculate() on both, sift::Matcher::match() on their points, then
// sift::Matcher::verify(): a RANSAC homography over the matches (include/sift/match.hpp; extensions, the reference has neither) -
// or, with model=fundamental, sift::Matcher::verify_fundamental(): a seven-point fundamental matrix, the model for two views of a
// general scene.  inliers.txt holds the lines of matches.txt that agree with the model.
//   g++ -std=c++17 -pthread -Iinclude examples/sift_verify.cpp -Lsift_amd/lib -lsift_hip -Wl,-rpath,$PWD/sift_amd/lib -o sift_verify
//   ./sift_verify a.pgm b.pgm [octaves=4] [dogsPerEpoch=3] [ratio=0.8] [crossCheck=0] [iterations=2048] [threshold=3] [seed=0] [refine=0] [model=homography|fundamental] [refit=-1] [localize=0] [warp|mosaic out.pgm [gain] [twoband]] [align N]
//   ... warp out.pgm (with model=homography): b registered onto a under the verified model (sift::Matcher::warp), as an 8-bit PGM
//   ... mosaic out.pgm (likewise; a and b of one size): both frames feathered on the canvas that holds them (sift::Matcher::composite)
//   ... mosaic out.pgm gain: the frames' gains are solved from their overlap first (sift::Matcher::overlap) and applied
//   ... mosaic out.pgm twoband: blended in two frequency bands of sigma 5 instead (sift::Matcher::composite_twoband), also after gain
//   ... align N (with model=homography, a and b of one size; last, or alone in place of warp|mosaic): the verified model refined on the
//       pixels by at most N Gauss-Newton steps (sift::Matcher::align) before it is printed, warped or composed
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "sift/match.hpp"
#include "sift/sift.hpp"

static std::vector<sift::InterestPoint> points_of(sift::Sift& sift, const std::string& file) {
    char err[512] = "";
    int w = 0, h = 0, bits = 0;
    if (sift_hip_image_info(file.c_str(), &w, &h, nullptr, &bits, err, sizeof(err)) != SIFT_HIP_OK) throw std::runtime_error(err);
    sift::Image2f img(w, h);
    if (sift_hip_image_read_band0(file.c_str(), img.data(), (long long)w * h, err, sizeof(err)) != SIFT_HIP_OK) throw std::runtime_error(err);
    if (bits != 8) return sift.calculate(img);
    std::vector<unsigned char> px((size_t)w * (size_t)h);   // an 8-bit file goes to the GPU as bytes (same floats, same result)
    for (size_t i = 0; i < px.size(); ++i) px[i] = (unsigned char)img.data()[i];
    return sift.calculate(px.data(), w, h);
}

static void write_matches(const char* path, const std::vector<sift::Match>& matches, const std::vector<unsigned char>* keep) {
    FILE* out = std::fopen(path, "w");
    if (!out) throw std::runtime_error(std::string("cannot write ") + path);
    for (size_t i = 0; i < matches.size(); ++i) {
        const sift::Match& m = matches[i];
        if (!keep || (*keep)[i]) std::fprintf(out, "%d %d %.9g %.9g\n", m.query, m.train, (double)m.dist2, (double)m.second2);
    }
    std::fclose(out);
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::cerr << "usage: " << argv[0]
                  << " a.{pgm,ppm,png,jpg} b.{...} [octaves] [dogsPerEpoch] [ratio] [crossCheck] [iterations] [threshold] [seed] [refine] [homography|fundamental] [refit] [localize] [warp|mosaic out.pgm [gain] [twoband]] [align N]\n";
        return 1;
    }
    const u16_t octaves = argc > 3 ? (u16_t)std::atoi(argv[3]) : 4;
    const u16_t dogsPerEpoch = argc > 4 ? (u16_t)std::atoi(argv[4]) : 3;
    const float ratio = argc > 5 ? (float)std::atof(argv[5]) : 0.8f;
    const bool crossCheck = argc > 6 && std::atoi(argv[6]) != 0;
    const unsigned iterations = argc > 7 ? (unsigned)std::atoi(argv[7]) : 2048u;
    const float threshold = argc > 8 ? (float)std::atof(argv[8]) : 3.0f;
    const unsigned seed = argc > 9 ? (unsigned)std::atoi(argv[9]) : 0u;
    const unsigned refine = argc > 10 ? (unsigned)std::atoi(argv[10]) : 0u;   // rounds of least-squares re-estimation over the inliers
    const std::string model_name = argc > 11 ? argv[11] : "homography";
    if (model_name != "homography" && model_name != "fundamental") {
        std::cerr << "model must be homography or fundamental\n";
        return 1;
    }
    // with model=fundamental: rounds of the least-squares refit of F (sift::Matcher::refine_fundamental), 0 .. 8; absent: no refit
    const int refit = argc > 12 ? std::atoi(argv[12]) : -1;
    // 1: the models are estimated on sub-pixel coordinates (sift::Sift::localize after each calculate, sift::Matcher::localize)
    const bool localize = argc > 13 && std::atoi(argv[13]) != 0;
    // "warp out.pgm": b resampled on a's pixel grid under the verified homography
    const std::string warp_file = argc > 15 && std::string(argv[14]) == "warp" ? argv[15] : "";
    // "mosaic out.pgm": a under the identity and b under the verified homography on one canvas
    const std::string mosaic_file = argc > 15 && std::string(argv[14]) == "mosaic" ? argv[15] : "";
    bool mosaic_gain = false, mosaic_twoband = false;   // "gain" and "twoband" after the file, in either order
    int align_rounds = 0;   // "align N" after everything else
    for (int k = 16; k < argc; ++k) {
        mosaic_gain |= std::string(argv[k]) == "gain";
        mosaic_twoband |= std::string(argv[k]) == "twoband";
    }
    for (int k = 14; k + 1 < argc; ++k)
        if (std::string(argv[k]) == "align") align_rounds = std::atoi(argv[k + 1]);
    if ((!warp_file.empty() || !mosaic_file.empty() || align_rounds) && model_name != "homography") {
        std::cerr << "warp, mosaic and align are for model=homography\n";
        return 1;
    }
    if (refit >= 0 && model_name != "fundamental") {
        std::cerr << "refit is for model=fundamental\n";
        return 1;
    }
    if (model_name == "fundamental" && refine) {
        std::cerr << "refine is for the homography: there is no least-squares refit of the fundamental matrix\n";
        return 1;
    }
    try {
        sift::Sift sift(dogsPerEpoch, octaves, 1.6f, std::sqrt(2.0f), false);
        const std::vector<sift::InterestPoint> a = points_of(sift, argv[1]);
        std::vector<sift_hip_localized> la, lb;
        if (localize) la = sift.localize();
        const std::vector<sift::InterestPoint> b = points_of(sift, argv[2]);
        if (localize) lb = sift.localize();
        sift::Matcher matcher;
        if (localize) matcher.localize(la, lb);
        const std::vector<sift::Match> matches = matcher.match(a, b, ratio, crossCheck);
        if (model_name == "fundamental") {
            sift::Fundamental model = matcher.verify_fundamental(a, b, matches, iterations, threshold, seed, false);
            int refitted = 0;
            if (refit >= 0) model = matcher.refine_fundamental(a, b, matches, model, threshold, refit, false, &refitted);
            write_matches("matches.txt", matches, nullptr);
            write_matches("inliers.txt", matches, &model.inlier);
            std::cout << a.size() << " and " << b.size() << " interest points, " << matches.size() << " matches -> matches.txt, " << model.inliers
                      << " inliers -> inliers.txt\n";
            if (refit >= 0) std::cout << "refitted " << refitted << " rounds\n";
            if (model.iteration < 0) {
                std::cout << "no fundamental matrix\n";
            } else {
                for (int r = 0; r < 3; ++r) std::printf("F %.9g %.9g %.9g\n", (double)model.f[3 * r], (double)model.f[3 * r + 1], (double)model.f[3 * r + 2]);
            }
            return 0;
        }
        sift::Homography model = matcher.verify(a, b, matches, iterations, threshold, seed, false, refine);
        write_matches("matches.txt", matches, nullptr);
        write_matches("inliers.txt", matches, &model.inlier);
        std::cout << a.size() << " and " << b.size() << " interest points, " << matches.size() << " matches -> matches.txt, " << model.inliers
                  << " inliers -> inliers.txt\n";
        if (refine) std::cout << "refined " << model.refined << " rounds\n";
        if (model.iteration < 0) {
            std::cout << "no homography\n";
        } else {
            for (int r = 0; r < 3; ++r) std::printf("H %.9g %.9g %.9g\n", (double)model.h[3 * r], (double)model.h[3 * r + 1], (double)model.h[3 * r + 2]);
        }
        if (align_rounds && model.iteration >= 0) {   // the model refined on the pixels; what follows takes the refined one
            char err[512] = "";
            int w = 0, h = 0, wb = 0, hb = 0;
            if (sift_hip_image_info(argv[1], &w, &h, nullptr, nullptr, err, sizeof(err)) != SIFT_HIP_OK ||
                sift_hip_image_info(argv[2], &wb, &hb, nullptr, nullptr, err, sizeof(err)) != SIFT_HIP_OK)
                throw std::runtime_error(err);
            if (w != wb || h != hb) throw std::runtime_error("align: the two images must have one size");
            sift::Image2f fa(w, h), fb(w, h);
            if (sift_hip_image_read_band0(argv[1], fa.data(), (long long)w * h, err, sizeof(err)) != SIFT_HIP_OK ||
                sift_hip_image_read_band0(argv[2], fb.data(), (long long)w * h, err, sizeof(err)) != SIFT_HIP_OK)
                throw std::runtime_error(err);
            const sift_hip_alignment al = matcher.align(fa, fb, model.h, align_rounds);
            std::printf("aligned %d rounds (status %d): rms %.4f -> %.4f over %d pixels, gain %.4f, bias %.3f\n", al.rounds, al.status, (double)al.rms0,
                        (double)al.rms, al.pixels, (double)al.gain, (double)al.bias);
            for (int r = 0; r < 3; ++r) std::printf("H %.9g %.9g %.9g\n", (double)model.h[3 * r], (double)model.h[3 * r + 1], (double)model.h[3 * r + 2]);
        }
        if (!warp_file.empty()) {   // no homography: the all-zero model covers nothing, the picture is black
            char err[512] = "";
            int wa = 0, ha = 0, wb = 0, hb = 0;
            if (sift_hip_image_info(argv[1], &wa, &ha, nullptr, nullptr, err, sizeof(err)) != SIFT_HIP_OK ||
                sift_hip_image_info(argv[2], &wb, &hb, nullptr, nullptr, err, sizeof(err)) != SIFT_HIP_OK)
                throw std::runtime_error(err);
            sift::Image2f train(wb, hb);
            if (sift_hip_image_read_band0(argv[2], train.data(), (long long)wb * hb, err, sizeof(err)) != SIFT_HIP_OK) throw std::runtime_error(err);
            sift::Image2f reg = matcher.warp(train, model.h, wa, ha);
            FILE* out = std::fopen(warp_file.c_str(), "wb");
            if (!out) throw std::runtime_error("cannot write " + warp_file);
            std::fprintf(out, "P5\n%d %d\n255\n", wa, ha);
            for (size_t i = 0; i < (size_t)wa * (size_t)ha; ++i) {   // rounded to nearest even and clamped, like the CLI's PNG
                const float v = std::nearbyint(reg.data()[i]);
                std::fputc((int)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v), out);
            }
            std::fclose(out);
            std::cout << argv[2] << " registered -> " << warp_file << "\n";
        }
        if (!mosaic_file.empty()) {   // no homography: the all-zero model covers nothing, the picture is a alone
            char err[512] = "";
            int w = 0, h = 0, wb = 0, hb = 0;
            if (sift_hip_image_info(argv[1], &w, &h, nullptr, nullptr, err, sizeof(err)) != SIFT_HIP_OK ||
                sift_hip_image_info(argv[2], &wb, &hb, nullptr, nullptr, err, sizeof(err)) != SIFT_HIP_OK)
                throw std::runtime_error(err);
            if (w != wb || h != hb) throw std::runtime_error("mosaic: the two images must have one size");
            sift::Image2f fa(w, h), fb(w, h);
            if (sift_hip_image_read_band0(argv[1], fa.data(), (long long)w * h, err, sizeof(err)) != SIFT_HIP_OK ||
                sift_hip_image_read_band0(argv[2], fb.data(), (long long)w * h, err, sizeof(err)) != SIFT_HIP_OK)
                throw std::runtime_error(err);
            // the canvas: a's frame and b's corners through the inverse model (adjugate, double), at most 4 x the larger side around a
            const double reach = 4.0 * std::max(w, h);
            double m[9], x0 = 0, y0 = 0, x1 = w - 1, y1 = h - 1;
            for (int k = 0; k < 9; ++k) m[k] = (double)model.h[k];
            const double adj[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                                   m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                                   m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
            for (int c = 0; c < 4 && model.iteration >= 0; ++c) {
                const double u = (c & 1) ? w - 1 : 0, v = (c & 2) ? h - 1 : 0, W = adj[6] * u + adj[7] * v + adj[8];
                const double x = (adj[0] * u + adj[1] * v + adj[2]) / W, y = (adj[3] * u + adj[4] * v + adj[5]) / W;
                if (!(std::isfinite(x) && std::isfinite(y))) continue;
                x0 = std::min(x0, std::floor(x)); x1 = std::max(x1, std::ceil(x));
                y0 = std::min(y0, std::floor(y)); y1 = std::max(y1, std::ceil(y));
            }
            x0 = std::max(x0, -reach); y0 = std::max(y0, -reach);
            x1 = std::min(x1, w - 1 + reach); y1 = std::min(y1, h - 1 + reach);
            const int cw = (int)(x1 - x0) + 1, ch = (int)(y1 - y0) + 1;
            std::array<f32_t, 9> ident = {1, 0, 0, 0, 1, 0, 0, 0, 1}, hb9;
            std::copy(model.h, model.h + 9, hb9.begin());
            sift::Matcher::Overlap ov;
            if (mosaic_gain) {
                ov = matcher.overlap({&fa, &fb}, {ident, hb9}, cw, ch, (int)x0, (int)y0);
                std::cout << "gains " << ov.gains[0] << ", " << ov.gains[1] << " over " << ov.stats[1] << " common pixels\n";
            }
            const std::vector<f32_t>* gains = mosaic_gain ? &ov.gains : nullptr;
            sift::Image2f pic = mosaic_twoband ? matcher.composite_twoband({&fa, &fb}, {ident, hb9}, cw, ch, (int)x0, (int)y0, 5.0f, 0.0f, true, nullptr, gains)
                                               : matcher.composite({&fa, &fb}, {ident, hb9}, cw, ch, (int)x0, (int)y0, 2, 0.0f, true, nullptr, gains);
            FILE* out = std::fopen(mosaic_file.c_str(), "wb");
            if (!out) throw std::runtime_error("cannot write " + mosaic_file);
            std::fprintf(out, "P5\n%d %d\n255\n", cw, ch);
            for (size_t i = 0; i < (size_t)cw * (size_t)ch; ++i) {
                const float v = std::nearbyint(pic.data()[i]);
                std::fputc((int)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v), out);
            }
            std::fclose(out);
            std::cout << argv[1] << " + " << argv[2] << " -> " << mosaic_file << " (" << cw << " x " << ch << ", origin " << (int)x0 << ", " << (int)y0 << ")\n";
        }
    } catch (std::exception& ex) {
        std::cerr << ex.what() << std::endl;
        return 2;
    }
    return 0;
}
