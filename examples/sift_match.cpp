// Two images -> matches.txt: sift::Sift::calculate() on both, sift::Matcher::match() on their points (include/sift/match.hpp; an
// extension, the reference has no matcher).  One line per match: `query train dist2 second2`, positions in the two point lists.
//   g++ -std=c++17 -pthread -Iinclude examples/sift_match.cpp -Lsift_amd/lib -lsift_hip -Wl,-rpath,$PWD/sift_amd/lib -o sift_match
//   ./sift_match a.pgm b.pgm [octaves=4] [dogsPerEpoch=3] [ratio=0.8] [crossCheck=0] [quantized=0]
// quantized=1: 8-bit descriptors, integer distances (the distances in matches.txt are then integers).
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

int main(int argc, char** argv) {
    if (argc < 3) {
        std::cerr << "usage: " << argv[0] << " a.{pgm,ppm,png,jpg} b.{...} [octaves] [dogsPerEpoch] [ratio] [crossCheck] [quantized]\n";
        return 1;
    }
    const u16_t octaves = argc > 3 ? (u16_t)std::atoi(argv[3]) : 4;
    const u16_t dogsPerEpoch = argc > 4 ? (u16_t)std::atoi(argv[4]) : 3;
    const float ratio = argc > 5 ? (float)std::atof(argv[5]) : 0.8f;
    const bool crossCheck = argc > 6 && std::atoi(argv[6]) != 0;
    const bool quantized = argc > 7 && std::atoi(argv[7]) != 0;
    try {
        sift::Sift sift(dogsPerEpoch, octaves, 1.6f, std::sqrt(2.0f), false);
        const std::vector<sift::InterestPoint> a = points_of(sift, argv[1]);
        const std::vector<sift::InterestPoint> b = points_of(sift, argv[2]);
        sift::Matcher matcher;
        const std::vector<sift::Match> matches = matcher.match(a, b, ratio, crossCheck, quantized);
        FILE* out = std::fopen("matches.txt", "w");
        if (!out) throw std::runtime_error("cannot write matches.txt");
        for (const sift::Match& m : matches) std::fprintf(out, "%d %d %.9g %.9g\n", m.query, m.train, (double)m.dist2, (double)m.second2);
        std::fclose(out);
        std::cout << a.size() << " and " << b.size() << " interest points, " << matches.size() << " matches -> matches.txt\n";
    } catch (std::exception& ex) {
        std::cerr << ex.what() << std::endl;
        return 2;
    }
    return 0;
}
