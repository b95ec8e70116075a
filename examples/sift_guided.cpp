// Two images -> matches.txt, inliers.txt and guided.txt: sift::Sift::calculate() on both, sift::Matcher::match() on their points,
// sift::Matcher::verify() or verify_fundamental() over the matches, then sift::Matcher::match_guided(): the points matched again,
// a point of b competing for a point of a only within `threshold` pixels of the verified model (include/sift/match.hpp;
// extensions, the reference has none of them).  guided.txt has the format of matches.txt; with no model it is empty.
//   g++ -std=c++17 -pthread -Iinclude examples/sift_guided.cpp -Lsift_amd/lib -lsift_hip -Wl,-rpath,$PWD/sift_amd/lib -o sift_guided
//   ./sift_guided a.pgm b.pgm [model=homography|fundamental] [octaves=4] [dogsPerEpoch=3] [ratio=0.8] [crossCheck=0] [iterations=2048] [threshold=3] [seed=0] [guidedRatio=ratio]
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
                  << " a.{pgm,ppm,png,jpg} b.{...} [homography|fundamental] [octaves] [dogsPerEpoch] [ratio] [crossCheck] [iterations] [threshold] [seed] [guidedRatio]\n";
        return 1;
    }
    const std::string model_name = argc > 3 ? argv[3] : "homography";
    const u16_t octaves = argc > 4 ? (u16_t)std::atoi(argv[4]) : 4;
    const u16_t dogsPerEpoch = argc > 5 ? (u16_t)std::atoi(argv[5]) : 3;
    const float ratio = argc > 6 ? (float)std::atof(argv[6]) : 0.8f;
    const bool crossCheck = argc > 7 && std::atoi(argv[7]) != 0;
    const unsigned iterations = argc > 8 ? (unsigned)std::atoi(argv[8]) : 2048u;
    const float threshold = argc > 9 ? (float)std::atof(argv[9]) : 3.0f;
    const unsigned seed = argc > 10 ? (unsigned)std::atoi(argv[10]) : 0u;
    const float guidedRatio = argc > 11 ? (float)std::atof(argv[11]) : ratio;
    if (model_name != "homography" && model_name != "fundamental") {
        std::cerr << "model must be homography or fundamental\n";
        return 1;
    }
    try {
        sift::Sift sift(dogsPerEpoch, octaves, 1.6f, std::sqrt(2.0f), false);
        const std::vector<sift::InterestPoint> a = points_of(sift, argv[1]);
        const std::vector<sift::InterestPoint> b = points_of(sift, argv[2]);
        sift::Matcher matcher;
        const std::vector<sift::Match> matches = matcher.match(a, b, ratio, crossCheck);
        write_matches("matches.txt", matches, nullptr);
        std::vector<sift::Match> guided;
        int inliers = 0;
        if (model_name == "fundamental") {
            const sift::Fundamental model = matcher.verify_fundamental(a, b, matches, iterations, threshold, seed, false);
            write_matches("inliers.txt", matches, &model.inlier);
            inliers = model.inliers;
            guided = matcher.match_guided(a, b, model, threshold, guidedRatio, crossCheck, false);
        } else {
            const sift::Homography model = matcher.verify(a, b, matches, iterations, threshold, seed, false, 0);
            write_matches("inliers.txt", matches, &model.inlier);
            inliers = model.inliers;
            guided = matcher.match_guided(a, b, model, threshold, guidedRatio, crossCheck, false);
        }
        write_matches("guided.txt", guided, nullptr);
        std::cout << a.size() << " and " << b.size() << " interest points, " << matches.size() << " matches -> matches.txt, " << inliers
                  << " inliers -> inliers.txt, " << guided.size() << " guided matches -> guided.txt\n";
    } catch (std::exception& ex) {
        std::cerr << ex.what() << std::endl;
        return 2;
    }
    return 0;
}
