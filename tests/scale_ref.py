"""The reference's scale schedule and its nearest-Gaussian search, restated in plain Python from the reference's source
(Sift::_createDOGs, sift.cpp:388-411, and Sift::_findNearestGaussian, sift.cpp:205-218) - not from the library's plan.

    schedule(dogs, octaves, sigma, k) -> (gauss_scale, dog_scale, nearest)

gauss_scale[o][j], j = 0 .. dogs, and dog_scale[o][i], i = 0 .. dogs - 1, are np.float32; nearest[o][i] = (octave, level) of the
Gaussian level a keypoint of DoG level (o, i) takes its gradient maps, orientation histogram and descriptor from.

The arithmetic, as the source has it:
  - `u16_t exp`, incremented once per level and `exp -= 2` between octaves (modulo 2^16, which dogs >= 3 never reaches);
  - `f32_t scale = std::pow(_k, exp) * _sigma`: std::pow(float, u16) promotes both to double, the product with the float
    sigma is formed in double and rounded to float once, by the assignment;
  - a DoG's scale is the float difference of two float scales; octave o + 1 starts from the scale of level (o, dogs - 1);
  - the search runs over the WHOLE pyramid, octave outer, level inner, `std::abs` of a float difference, strict `<` from an
    initial 100: the first of equal differences wins, and a difference of 100 or more selects (0, 0).
"""
import math

import numpy as np

f32 = np.float32


def schedule(dogs, octaves, sigma, k):
    sigma, k = f32(sigma), f32(k)
    gauss = [[None] * (dogs + 1) for _ in range(octaves)]
    dog = [[None] * dogs for _ in range(octaves)]
    gauss[0][0] = sigma
    exp = 0
    for o in range(octaves):
        for j in range(1, dogs + 1):
            gauss[o][j] = f32(math.pow(float(k), float(exp)) * float(sigma))
            dog[o][j - 1] = f32(gauss[o][j] - gauss[o][j - 1])
            exp = (exp + 1) & 0xffff
        if o < octaves - 1:
            gauss[o + 1][0] = gauss[o][dogs - 1]
            exp = (exp - 2) & 0xffff
    nearest = [[find_nearest_gaussian(gauss, s) for s in row] for row in dog]
    return gauss, dog, nearest


def find_nearest_gaussian(gauss, scale):
    lowest, best = f32(100), (0, 0)
    for o, row in enumerate(gauss):
        for i, g in enumerate(row):
            cur = f32(abs(f32(g - f32(scale))))
            if cur < lowest:
                lowest, best = cur, (o, i)
    return best


def level_populations(points, nearest):
    """{(octave, level): how many of `points` (records with `octave` and `index` fields) select that Gaussian level}."""
    out = {}
    for o, i in zip(points["octave"].tolist(), points["index"].tolist()):
        out[nearest[o][i]] = out.get(nearest[o][i], 0) + 1
    return out
