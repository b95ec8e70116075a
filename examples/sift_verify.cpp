// Two images -> matches.txt and inliers.txt: sift::Sift::calculate() on both, sift::Matcher::match() on their points, then
// sift::Matcher::verify(): a RANSAC homography over the matches (include/sift/match.hpp; extensions, the reference has neither) -
// or, with model=fundamental, sift::Matcher::verify_fundamental(): a seven-point fundamental matrix, the model for two views of a
// general scene.  inliers.txt holds the lines of matches.txt that agree with the model.
//   g++ -std=c++17 -pthread -Iinclude examples/sift_verify.cpp -Lsift_amd/lib -lsift_hip -Wl,-rpath,$PWD/sift_amd/lib -o sift_verify
//   ./sift_verify a.pgm b.pgm [octaves=4] [dogsPerEpoch=3] [ratio=0.8] [crossCheck=0] [iterations=2048] [threshold=3] [seed=0] [refine=0] [model=homography|fundamental]
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
                  << " a.{pgm,ppm,png,jpg} b.{...} [octaves] [dogsPerEpoch] [ratio] [crossCheck] [iterations] [threshold] [seed] [refine] [homography|fundamental]\n";
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
    if (model_name == "fundamental" && refine) {
        std::cerr << "refine is for the homography: there is no least-squares refit of the fundamental matrix\n";
        return 1;
    }
    try {
        sift::Sift sift(dogsPerEpoch, octaves, 1.6f, std::sqrt(2.0f), false);
        const std::vector<sift::InterestPoint> a = points_of(sift, argv[1]);
        const std::vector<sift::InterestPoint> b = points_of(sift, argv[2]);
        sift::Matcher matcher;
        const std::vector<sift::Match> matches = matcher.match(a, b, ratio, crossCheck);
        if (model_name == "fundamental") {
            const sift::Fundamental model = matcher.verify_fundamental(a, b, matches, iterations, threshold, seed, false);
            write_matches("matches.txt", matches, nullptr);
            write_matches("inliers.txt", matches, &model.inlier);
            std::cout << a.size() << " and " << b.size() << " interest points, " << matches.size() << " matches -> matches.txt, " << model.inliers
                      << " inliers -> inliers.txt\n";
            if (model.iteration < 0) {
                std::cout << "no fundamental matrix\n";
            } else {
                for (int r = 0; r < 3; ++r) std::printf("F %.9g %.9g %.9g\n", (double)model.f[3 * r], (double)model.f[3 * r + 1], (double)model.f[3 * r + 2]);
            }
            return 0;
        }
        const sift::Homography model = matcher.verify(a, b, matches, iterations, threshold, seed, false, refine);
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
    } catch (std::exception& ex) {
        std::cerr << ex.what() << std::endl;
        return 2;
    }
    return 0;
}
