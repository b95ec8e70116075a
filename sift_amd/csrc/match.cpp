// Host side of descriptor matching (include/sift_hip.h: sift_hip_knn2, sift_hip_match, sift_hip_result_match, and their guided
// counterparts sift_hip_knn2_guided, sift_hip_match_guided, sift_hip_result_match_guided): staging of
// caller memory, the tile table that makes many pairs one launch, and the scratch memory, which the first match call of a
// context allocates and the context keeps - outside the batch arena, so a context that never matches allocates nothing here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "match_kernels.h"
#include "ransac_kernels.h"   // match_result_on_device

namespace sift_hip {

struct MatchState {
    ScratchBuf d_desc, d_kp;                 // staging of descriptor rows / keypoint records that arrive in host memory
    ScratchBuf d_norm, d_valid;              // n(a) and the valid flag of every row
    ScratchBuf d_tiles, d_blocks, d_pairs;   // the launch tables
    ScratchBuf d_part;                       // partial top-2s, kMatchQ per tile
    ScratchBuf d_idx, d_dist;                // top-2 of every query row (forward rows first, then the cross-check's reverse rows)
    ScratchBuf d_seg, d_out, d_counts;       // records per pair segment, the dense list, per-pair counts
    ScratchBuf d_xy, d_models;               // guided matching: the rows' points (staged, or built from the keypoints), the pairs' models
    ScratchBuf d_desc8;                      // 8-bit rows: staged from host memory, or quantised from the float rows (params->quantized)
    void* h_tables = nullptr;         // page-locked image of the three tables (the copy is asynchronous)
    size_t h_cap = 0;
    std::vector<int32_t> counts;
};

void match_state_free(MatchState* st) {
    if (!st) return;
    for (ScratchBuf* b : {&st->d_desc, &st->d_kp, &st->d_norm, &st->d_valid, &st->d_tiles, &st->d_blocks, &st->d_pairs, &st->d_part, &st->d_idx,
                   &st->d_dist, &st->d_seg, &st->d_out, &st->d_counts, &st->d_xy, &st->d_models, &st->d_desc8})
        b->release();
    if (st->h_tables) {
        ApiGuard api;
        (void)hipHostFree(st->h_tables);
    }
    delete st;
}

namespace {

struct Job {
    sift_hip_ctx* c;
    const float* desc;
    const sift_hip_keypoint* kp;
    bool inputs_on_device;   // sift_hip_result_match: the context's own arrays
    int n_sets;
    const int64_t* offsets;
    int n_pairs;
    const int32_t *pair_q, *pair_t;
    const sift_hip_match_params* params;   // null: top-2 only
    int32_t* idx;
    float* dist2;
    sift_hip_match_rec* recs;
    int32_t* counts;
    int64_t* total;
    char* err;
    int errlen;
    // sift_hip_result_verify goes on with the list where it is: the dense records on the device, the pairs' counts (both null: not asked)
    const sift_hip_match_rec** d_recs_out = nullptr;
    int32_t* host_counts_out = nullptr;
    // guided matching (guided: all three must be given, except that sift_hip_result_match_guided builds xy from the keypoints)
    bool guided = false;
    const float* xy = nullptr;
    const sift_hip_guide_params* guide = nullptr;
    const float* models = nullptr;
    float coord_scale = 1.0f;   // the result call's: 0.5f after a batch with subpixel
    const uint8_t* desc8 = nullptr;   // sift_hip_knn2_u8 / sift_hip_match_u8: byte rows in place of `desc`
    bool is_u8 = false;
};

int fail(const Job& j, const char* msg) {
    match_set_err(j.err, j.errlen, msg);
    return SIFT_HIP_EINVAL;
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// the tiles of one (query set, train set): blocks of kMatchQ query rows, each against `splits` ranges of the train set
void add_tiles(long long q0, long long nq, long long t0, long long nt, int target_tiles_per_block, int out_row0, int pair_dir,
               std::vector<MatchTile>& tiles, std::vector<MatchBlock>& blocks) {
    const long long stages = (nt + kMatchT - 1) / kMatchT;
    const long long stages_per_split_min = kMatchSplitRows / kMatchT;
    long long splits = std::max<long long>(1, std::min<long long>(target_tiles_per_block, (nt + kMatchSplitRows - 1) / kMatchSplitRows));
    long long per = (stages + splits - 1) / std::max<long long>(splits, 1);
    per = (per + stages_per_split_min - 1) / stages_per_split_min * stages_per_split_min;   // split edges at multiples of kMatchSplitRows
    for (long long b = 0; b * kMatchQ < nq; ++b) {
        MatchBlock blk{};
        blk.q_row0 = (int)(q0 + b * kMatchQ);
        blk.q_rows = (int)std::min<long long>(kMatchQ, nq - b * kMatchQ);
        blk.out_row0 = out_row0 + (int)(b * kMatchQ);
        blk.first_tile = (int)tiles.size();
        for (long long s0 = 0; s0 < stages; s0 += per) {
            MatchTile t{};
            t.q_row0 = blk.q_row0;
            t.q_rows = blk.q_rows;
            t.t_set0 = (int)t0;
            t.t_lo = (int)(s0 * kMatchT);
            t.t_hi = (int)std::min<long long>(nt, (s0 + per) * kMatchT);
            t.pair_dir = pair_dir;
            tiles.push_back(t);
        }
        blk.n_tiles = (int)tiles.size() - blk.first_tile;
        blocks.push_back(blk);
    }
}

int run(void* arg) {
    const Job& j = *static_cast<const Job*>(arg);
    MatchCtxView v = match_ctx_view(j.c);
    SIFT_HIP_CHECK(hipSetDevice(v.device));

    // ---- arguments ----
    if (j.n_sets < 0 || j.n_pairs < 0 || (j.n_sets > 0 && !j.offsets) || (j.n_pairs > 0 && (!j.pair_q || !j.pair_t)))
        return fail(j, "sift_hip match: bad set or pair arguments");
    const long long rows = j.n_sets > 0 ? (long long)j.offsets[j.n_sets] : 0;
    if (j.n_sets > 0 && j.offsets[0] < 0) return fail(j, "sift_hip match: offsets must start at >= 0");
    for (int s = 0; s < j.n_sets; ++s)
        if (j.offsets[s + 1] < j.offsets[s]) return fail(j, "sift_hip match: offsets must ascend");
    if (rows > 0x7fffffffLL / 2) return fail(j, "sift_hip match: too many rows");
    if (rows > 0 && !(j.is_u8 ? (const void*)j.desc8 : (const void*)j.desc)) return fail(j, "sift_hip match: no descriptors");
    bool use_ratio = false, cross = false, quantized = false;
    float ratio2 = 0.0f;
    if (j.params) {
        if (j.params->quantized > 1) return fail(j, "sift_hip match: quantized must be 0 (float rows) or 1 (8-bit rows, integer distances)");
        quantized = j.params->quantized == 1;
        if (quantized && j.guided) return fail(j, "sift_hip match: quantized = 1 is not available in guided matching (float rows only)");
        const float r = j.params->ratio;
        if (!(r >= 0.0f && r <= 1.0f)) return fail(j, "sift_hip match: ratio must be 0 (no ratio test) or in (0, 1]");
        use_ratio = r != 0.0f;
        ratio2 = r * r;
        cross = j.params->cross_check != 0;
    }
    if (j.guided) {
        if (!j.guide) return fail(j, "sift_hip match: no guide parameters");
        if (j.guide->model != SIFT_HIP_GUIDE_HOMOGRAPHY && j.guide->model != SIFT_HIP_GUIDE_FUNDAMENTAL)
            return fail(j, "sift_hip match: guide model must be 0 (homography) or 1 (fundamental)");
        if (!(std::isfinite(j.guide->threshold) && j.guide->threshold > 0.0f)) return fail(j, "sift_hip match: guide threshold must be finite and > 0");
        if (!j.models) return fail(j, "sift_hip match: no models");
        if (!j.xy && !j.inputs_on_device) return fail(j, "sift_hip match: no coordinates");
        if (j.n_pairs > 0x3fffffff) return fail(j, "sift_hip match: too many pairs");
    }
    long long fwd_rows = 0, rev_rows = 0;
    for (int p = 0; p < j.n_pairs; ++p) {
        const int q = j.pair_q[p], t = j.pair_t[p];
        if (q < 0 || q >= j.n_sets || t < 0 || t >= j.n_sets) return fail(j, "sift_hip match: pair names a set that does not exist");
        fwd_rows += j.offsets[q + 1] - j.offsets[q];
        if (cross) rev_rows += j.offsets[t + 1] - j.offsets[t];
    }
    if (fwd_rows + rev_rows > 0x7fffffffLL / 2) return fail(j, "sift_hip match: too many query rows");
    if (j.params ? (fwd_rows > 0 && !j.recs) : (fwd_rows > 0 && (!j.idx || !j.dist2))) return fail(j, "sift_hip match: no result array");

    if (j.counts) std::fill(j.counts, j.counts + j.n_pairs, 0);
    if (j.total) *j.total = 0;
    if (j.d_recs_out) *j.d_recs_out = nullptr;
    if (j.host_counts_out) std::fill(j.host_counts_out, j.host_counts_out + j.n_pairs, 0);
    if (fwd_rows == 0) return SIFT_HIP_OK;

    if (!*v.state) *v.state = new MatchState();
    MatchState& st = **v.state;

    // ---- inputs on the device ----
    const float* d_desc = j.desc;
    const uint8_t* d_desc8 = j.desc8;
    const sift_hip_keypoint* d_kp = j.kp;
    if (!j.inputs_on_device) {
        if (j.is_u8) {
            if (!match_ptr_on_device(j.desc8)) {
                st.d_desc8.ensure((size_t)rows * 128);
                match_upload(j.c, st.d_desc8.p, j.desc8, (size_t)rows * 128);
                match_wait(j.c);
                d_desc8 = st.d_desc8.as<uint8_t>();
            } else if (reinterpret_cast<uintptr_t>(j.desc8) % 16 != 0) {
                return fail(j, "sift_hip match: 8-bit rows in device memory must be aligned to 16 bytes");
            }
        } else if (!match_ptr_on_device(j.desc)) {
            st.d_desc.ensure((size_t)rows * 128 * sizeof(float));
            match_upload(j.c, st.d_desc.p, j.desc, (size_t)rows * 128 * sizeof(float));
            match_wait(j.c);   // pageable memory travels through the context's two staging buffers: the next upload refills them
            d_desc = st.d_desc.as<float>();
        }
        if (j.kp && !match_ptr_on_device(j.kp)) {
            st.d_kp.ensure((size_t)rows * sizeof(sift_hip_keypoint));
            match_upload(j.c, st.d_kp.p, j.kp, (size_t)rows * sizeof(sift_hip_keypoint));
            d_kp = st.d_kp.as<sift_hip_keypoint>();
        }
    }
    MatchGuideArgs ga;
    if (j.guided) {
        ga.thr2 = j.guide->threshold * j.guide->threshold;
        ga.xy = j.xy;
        if (j.inputs_on_device) {   // the context's keypoints: every row's point is built on the device
            st.d_xy.ensure((size_t)rows * 2 * sizeof(float));
            launch_match_coords(v.stream, d_kp, rows, j.coord_scale, st.d_xy.as<float>());
            ga.xy = st.d_xy.as<float>();
        } else if (!match_ptr_on_device(j.xy)) {
            match_wait(j.c);   // the staging buffers may still hold the keypoints
            st.d_xy.ensure((size_t)rows * 2 * sizeof(float));
            match_upload(j.c, st.d_xy.p, j.xy, (size_t)rows * 2 * sizeof(float));
            match_wait(j.c);
            ga.xy = st.d_xy.as<float>();
        }
        ga.models = j.models;
        if (!match_ptr_on_device(j.models)) {
            match_wait(j.c);
            st.d_models.ensure((size_t)j.n_pairs * 9 * sizeof(float));
            match_upload(j.c, st.d_models.p, j.models, (size_t)j.n_pairs * 9 * sizeof(float));
            match_wait(j.c);
            ga.models = st.d_models.as<float>();
        }
    }

    // ---- the tables: every pair's tiles (and, for the cross-check, those of the pair with its roles swapped) ----
    long long q_blocks = 0;
    for (int p = 0; p < j.n_pairs; ++p) {
        const long long nq = j.offsets[j.pair_q[p] + 1] - j.offsets[j.pair_q[p]], nt = j.offsets[j.pair_t[p] + 1] - j.offsets[j.pair_t[p]];
        q_blocks += (nq + kMatchQ - 1) / kMatchQ + (cross ? (nt + kMatchQ - 1) / kMatchQ : 0);
    }
    // one workgroup occupies a CU (LDS); with fewer than about four rounds of them the last round's idle CUs show, so below
    // that the train sets are split further
    const int want = 4 * resident_cus();
    const int per_block = (int)std::max<long long>(1, (want + q_blocks - 1) / std::max<long long>(q_blocks, 1));
    std::vector<MatchTile> tiles;
    std::vector<MatchBlock> blocks;
    std::vector<MatchPair> pairs((size_t)j.n_pairs);
    long long out_row = 0, rev_row = fwd_rows;
    for (int p = 0; p < j.n_pairs; ++p) {
        const long long q0 = j.offsets[j.pair_q[p]], nq = j.offsets[j.pair_q[p] + 1] - q0;
        const long long t0 = j.offsets[j.pair_t[p]], nt = j.offsets[j.pair_t[p] + 1] - t0;
        pairs[(size_t)p] = MatchPair{(int)out_row, (int)nq, cross ? (int)rev_row : -1, 0};
        add_tiles(q0, nq, t0, nt, per_block, (int)out_row, j.guided ? 2 * p : 0, tiles, blocks);
        out_row += nq;
        if (cross) {
            add_tiles(t0, nt, q0, nq, per_block, (int)rev_row, j.guided ? 2 * p + 1 : 0, tiles, blocks);
            rev_row += nt;
        }
    }
    const long long all_rows = fwd_rows + rev_rows;

    const size_t b_tiles = align256(tiles.size() * sizeof(MatchTile)), b_blocks = align256(blocks.size() * sizeof(MatchBlock)),
                 b_pairs = align256(pairs.size() * sizeof(MatchPair));
    if (b_tiles + b_blocks + b_pairs > st.h_cap) {
        ApiGuard api;
        if (st.h_tables) SIFT_HIP_CHECK(hipHostFree(st.h_tables));
        st.h_tables = nullptr;
        st.h_cap = 0;
        SIFT_HIP_CHECK(hipHostMalloc(&st.h_tables, 2 * (b_tiles + b_blocks + b_pairs), hipHostMallocDefault));
        st.h_cap = 2 * (b_tiles + b_blocks + b_pairs);
    }
    char* h = static_cast<char*>(st.h_tables);
    std::memcpy(h, tiles.data(), tiles.size() * sizeof(MatchTile));
    std::memcpy(h + b_tiles, blocks.data(), blocks.size() * sizeof(MatchBlock));
    std::memcpy(h + b_tiles + b_blocks, pairs.data(), pairs.size() * sizeof(MatchPair));
    st.d_tiles.ensure(b_tiles);
    st.d_blocks.ensure(b_blocks);
    st.d_pairs.ensure(b_pairs);
    if (!tiles.empty()) SIFT_HIP_CHECK(hipMemcpyAsync(st.d_tiles.p, h, b_tiles, hipMemcpyHostToDevice, v.stream));
    SIFT_HIP_CHECK(hipMemcpyAsync(st.d_blocks.p, h + b_tiles, b_blocks, hipMemcpyHostToDevice, v.stream));
    SIFT_HIP_CHECK(hipMemcpyAsync(st.d_pairs.p, h + b_tiles + b_blocks, b_pairs, hipMemcpyHostToDevice, v.stream));

    const bool u8 = j.is_u8 || quantized;
    if (quantized && !j.is_u8) {   // the float rows become bytes on the device, in the pass that forms their norms
        st.d_desc8.ensure((size_t)rows * 128);
        d_desc8 = st.d_desc8.as<uint8_t>();
    }
    st.d_norm.ensure((size_t)rows * sizeof(float));
    st.d_valid.ensure((size_t)rows);
    st.d_part.ensure(std::max<size_t>(tiles.size(), 1) * kMatchQ * sizeof(MatchTop2));
    const bool idx_direct = !j.params && match_ptr_on_device(j.idx), dist_direct = !j.params && match_ptr_on_device(j.dist2);
    if (!idx_direct) st.d_idx.ensure((size_t)all_rows * 2 * sizeof(int32_t));
    if (!dist_direct) st.d_dist.ensure((size_t)all_rows * 2 * sizeof(float));
    int32_t* d_idx = idx_direct ? j.idx : st.d_idx.as<int32_t>();
    float* d_dist = dist_direct ? j.dist2 : st.d_dist.as<float>();

    // ---- the launches: one of each kernel, whatever the number of pairs ----
    if (u8) {
        if (j.is_u8)
            launch_match_norms_u8(v.stream, d_desc8, d_kp, rows, st.d_norm.as<int32_t>(), st.d_valid.as<uint8_t>());
        else
            launch_match_quantize_norms(v.stream, d_desc, d_kp, rows, st.d_desc8.as<uint8_t>(), st.d_norm.as<int32_t>(), st.d_valid.as<uint8_t>());
        launch_match_tiles_u8(v.stream, d_desc8, st.d_norm.as<int32_t>(), st.d_valid.as<uint8_t>(), st.d_tiles.as<MatchTile>(), (int)tiles.size(),
                              st.d_part.as<MatchTop2>());
    } else {
        launch_match_norms(v.stream, d_desc, d_kp, rows, st.d_norm.as<float>(), st.d_valid.as<uint8_t>());
        if (j.guided)
            launch_match_tiles_guided(v.stream, d_desc, st.d_norm.as<float>(), st.d_valid.as<uint8_t>(), st.d_tiles.as<MatchTile>(),
                                      (int)tiles.size(), st.d_part.as<MatchTop2>(), (int)j.guide->model, ga);
        else
            launch_match_tiles(v.stream, d_desc, st.d_norm.as<float>(), st.d_valid.as<uint8_t>(), st.d_tiles.as<MatchTile>(), (int)tiles.size(),
                               st.d_part.as<MatchTop2>());
    }
    launch_match_merge(v.stream, st.d_part.as<MatchTop2>(), st.d_valid.as<uint8_t>(), st.d_blocks.as<MatchBlock>(), (int)blocks.size(), d_idx,
                       d_dist);
    SIFT_HIP_CHECK(hipGetLastError());

    if (!j.params) {
        if (!idx_direct) match_download(j.c, j.idx, d_idx, (size_t)fwd_rows * 2 * sizeof(int32_t));
        if (!dist_direct) match_download(j.c, j.dist2, d_dist, (size_t)fwd_rows * 2 * sizeof(float));
        match_wait(j.c);
        return SIFT_HIP_OK;
    }

    const bool recs_direct = match_ptr_on_device(j.recs);
    st.d_seg.ensure((size_t)fwd_rows * sizeof(sift_hip_match_rec));
    st.d_counts.ensure((size_t)j.n_pairs * sizeof(int32_t));
    if (!recs_direct) st.d_out.ensure((size_t)fwd_rows * sizeof(sift_hip_match_rec));
    sift_hip_match_rec* d_out = recs_direct ? j.recs : st.d_out.as<sift_hip_match_rec>();
    launch_match_filter(v.stream, d_idx, d_dist, st.d_pairs.as<MatchPair>(), j.n_pairs, use_ratio ? 1 : 0, ratio2, cross ? 1 : 0,
                        st.d_seg.as<sift_hip_match_rec>(), st.d_counts.as<int32_t>());
    launch_match_pack(v.stream, st.d_seg.as<sift_hip_match_rec>(), st.d_pairs.as<MatchPair>(), st.d_counts.as<int32_t>(), j.n_pairs, d_out);
    SIFT_HIP_CHECK(hipGetLastError());
    st.counts.assign((size_t)j.n_pairs, 0);
    match_download(j.c, st.counts.data(), st.d_counts.p, (size_t)j.n_pairs * sizeof(int32_t));
    long long total = 0;
    for (int32_t n : st.counts) total += n;
    if (!recs_direct && total > 0) match_download(j.c, j.recs, d_out, (size_t)total * sizeof(sift_hip_match_rec));
    match_wait(j.c);
    if (j.counts) std::copy(st.counts.begin(), st.counts.end(), j.counts);
    if (j.total) *j.total = total;
    if (j.d_recs_out) *j.d_recs_out = d_out;
    if (j.host_counts_out) std::copy(st.counts.begin(), st.counts.end(), j.host_counts_out);
    return SIFT_HIP_OK;
}

// sift_hip_quantize and sift_hip_result_copy_u8: float rows (caller memory, or the context's results) -> byte rows in caller memory
struct QuantizeJob {
    sift_hip_ctx* c;
    const float* desc;
    bool from_result;
    long long rows;
    uint8_t* out;
    char* err;
    int errlen;
};

int run_quantize(void* arg) {
    const QuantizeJob& j = *static_cast<const QuantizeJob*>(arg);
    MatchCtxView v = match_ctx_view(j.c);
    SIFT_HIP_CHECK(hipSetDevice(v.device));
    if (j.rows <= 0) return SIFT_HIP_OK;
    const bool in_on_device = j.from_result || match_ptr_on_device(j.desc), direct = match_ptr_on_device(j.out);
    if ((in_on_device && reinterpret_cast<uintptr_t>(j.desc) % 16 != 0) || (direct && reinterpret_cast<uintptr_t>(j.out) % 16 != 0)) {
        match_set_err(j.err, j.errlen, "sift_hip quantize: rows in device memory must be aligned to 16 bytes");
        return SIFT_HIP_EINVAL;
    }
    if (!*v.state) *v.state = new MatchState();
    MatchState& st = **v.state;
    const float* d_desc = j.desc;
    if (!in_on_device) {
        st.d_desc.ensure((size_t)j.rows * 128 * sizeof(float));
        match_upload(j.c, st.d_desc.p, j.desc, (size_t)j.rows * 128 * sizeof(float));
        match_wait(j.c);
        d_desc = st.d_desc.as<float>();
    }
    if (!direct) st.d_desc8.ensure((size_t)j.rows * 128);
    uint8_t* d_out = direct ? j.out : st.d_desc8.as<uint8_t>();
    launch_match_quantize(v.stream, d_desc, j.rows, d_out);
    SIFT_HIP_CHECK(hipGetLastError());
    if (!direct) match_download(j.c, j.out, d_out, (size_t)j.rows * 128);
    match_wait(j.c);
    return SIFT_HIP_OK;
}

}  // namespace
}  // namespace sift_hip

namespace sift_hip {
int match_result_on_device(sift_hip_ctx* c, const char* who, int n_pairs, const int32_t* pair_q, const int32_t* pair_t,
                           const sift_hip_match_params* params, sift_hip_match_rec* recs, int32_t* counts, int64_t* total,
                           const sift_hip_match_rec** d_recs, int32_t* host_counts, char* err, int errlen) {
    const MatchCtxView v = match_ctx_view(c);
    if (!v.have_result) {
        match_set_err(err, errlen, (std::string(who) + ": the context holds no results").c_str());
        return SIFT_HIP_EINVAL;
    }
    std::vector<int64_t> offsets((size_t)v.n_images + 1, 0);
    for (int i = 0; i < v.n_images; ++i) offsets[(size_t)i + 1] = offsets[(size_t)i] + v.counts[i];
    Job j{c, v.d_desc, v.d_kp, true, v.n_images, offsets.data(), n_pairs, pair_q, pair_t, params, nullptr, nullptr, recs, counts, total, err, errlen,
          d_recs, host_counts};
    return match_guarded(err, errlen, run, &j);
}
}  // namespace sift_hip

// sift_hip_result_match_guided: the images' rows of the device-resident results, their points built from the keypoints
static int result_match_guided(sift_hip_ctx* c, int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* params,
                               const sift_hip_guide_params* guide, const float* models, sift_hip_match_rec* recs, int32_t* counts, int64_t* total,
                               char* err, int errlen) {
    using namespace sift_hip;
    const MatchCtxView v = match_ctx_view(c);
    if (!v.have_result) {
        match_set_err(err, errlen, "sift_hip_result_match_guided: the context holds no results");
        return SIFT_HIP_EINVAL;
    }
    std::vector<int64_t> offsets((size_t)v.n_images + 1, 0);
    for (int i = 0; i < v.n_images; ++i) offsets[(size_t)i + 1] = offsets[(size_t)i] + v.counts[i];
    Job j{c, v.d_desc, v.d_kp, true, v.n_images, offsets.data(), n_pairs, pair_q, pair_t, params, nullptr, nullptr, recs, counts, total, err, errlen};
    j.guided = true;
    j.guide = guide;
    j.models = models;
    j.coord_scale = ransac_ctx_subpixel(c) ? 0.5f : 1.0f;
    return match_guarded(err, errlen, run, &j);
}

using namespace sift_hip;

extern "C" {

int sift_hip_knn2(sift_hip_ctx* c, const float* desc, const sift_hip_keypoint* kp, int n_sets, const int64_t* offsets, int n_pairs,
                  const int32_t* pair_q, const int32_t* pair_t, int32_t* idx, float* dist2, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_knn2: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, desc, kp, false, n_sets, offsets, n_pairs, pair_q, pair_t, nullptr, idx, dist2, nullptr, nullptr, nullptr, err, errlen};
    return match_guarded(err, errlen, run, &j);
}

int sift_hip_match(sift_hip_ctx* c, const float* desc, const sift_hip_keypoint* kp, int n_sets, const int64_t* offsets, int n_pairs,
                   const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* params, sift_hip_match_rec* recs,
                   int32_t* counts, int64_t* total, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_match: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    if (!params) { match_set_err(err, errlen, "sift_hip_match: no parameters"); return SIFT_HIP_EINVAL; }
    Job j{c, desc, kp, false, n_sets, offsets, n_pairs, pair_q, pair_t, params, nullptr, nullptr, recs, counts, total, err, errlen};
    return match_guarded(err, errlen, run, &j);
}

int sift_hip_result_match(sift_hip_ctx* c, int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* params,
                          sift_hip_match_rec* recs, int32_t* counts, int64_t* total, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_result_match: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    if (!params) { match_set_err(err, errlen, "sift_hip_result_match: no parameters"); return SIFT_HIP_EINVAL; }
    return match_result_on_device(c, "sift_hip_result_match", n_pairs, pair_q, pair_t, params, recs, counts, total, nullptr, nullptr, err, errlen);
}

int sift_hip_knn2_guided(sift_hip_ctx* c, const float* desc, const sift_hip_keypoint* kp, const float* xy, int n_sets, const int64_t* offsets,
                         int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_guide_params* guide, const float* models,
                         int32_t* idx, float* dist2, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_knn2_guided: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, desc, kp, false, n_sets, offsets, n_pairs, pair_q, pair_t, nullptr, idx, dist2, nullptr, nullptr, nullptr, err, errlen};
    j.guided = true;
    j.xy = xy;
    j.guide = guide;
    j.models = models;
    return match_guarded(err, errlen, run, &j);
}

int sift_hip_match_guided(sift_hip_ctx* c, const float* desc, const sift_hip_keypoint* kp, const float* xy, int n_sets, const int64_t* offsets,
                          int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* params,
                          const sift_hip_guide_params* guide, const float* models, sift_hip_match_rec* recs, int32_t* counts, int64_t* total,
                          char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_match_guided: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    if (!params) { match_set_err(err, errlen, "sift_hip_match_guided: no parameters"); return SIFT_HIP_EINVAL; }
    Job j{c, desc, kp, false, n_sets, offsets, n_pairs, pair_q, pair_t, params, nullptr, nullptr, recs, counts, total, err, errlen};
    j.guided = true;
    j.xy = xy;
    j.guide = guide;
    j.models = models;
    return match_guarded(err, errlen, run, &j);
}

int sift_hip_result_match_guided(sift_hip_ctx* c, int n_pairs, const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* params,
                                 const sift_hip_guide_params* guide, const float* models, sift_hip_match_rec* recs, int32_t* counts,
                                 int64_t* total, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_result_match_guided: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    if (!params) { match_set_err(err, errlen, "sift_hip_result_match_guided: no parameters"); return SIFT_HIP_EINVAL; }
    return result_match_guided(c, n_pairs, pair_q, pair_t, params, guide, models, recs, counts, total, err, errlen);
}

int sift_hip_quantize(sift_hip_ctx* c, const float* desc, int64_t rows, uint8_t* out, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_quantize: no context (the quantiser runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    if (rows < 0 || rows > 0x7fffffffLL / 2) { match_set_err(err, errlen, "sift_hip_quantize: bad number of rows"); return SIFT_HIP_EINVAL; }
    if (rows > 0 && (!desc || !out)) { match_set_err(err, errlen, "sift_hip_quantize: no rows or no result array"); return SIFT_HIP_EINVAL; }
    QuantizeJob j{c, desc, false, (long long)rows, out, err, errlen};
    return match_guarded(err, errlen, run_quantize, &j);
}

int sift_hip_result_copy_u8(sift_hip_ctx* c, uint8_t* descriptors) {
    if (!c) return SIFT_HIP_EINVAL;
    const MatchCtxView v = match_ctx_view(c);
    if (!v.have_result) return SIFT_HIP_EINVAL;
    long long total = 0;
    for (int i = 0; i < v.n_images; ++i) total += v.counts[i];
    if (total <= 0 || !descriptors) return SIFT_HIP_OK;
    QuantizeJob j{c, v.d_desc, true, total, descriptors, nullptr, 0};
    return match_guarded(nullptr, 0, run_quantize, &j);
}

int sift_hip_knn2_u8(sift_hip_ctx* c, const uint8_t* desc, const sift_hip_keypoint* kp, int n_sets, const int64_t* offsets, int n_pairs,
                     const int32_t* pair_q, const int32_t* pair_t, int32_t* idx, float* dist2, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_knn2_u8: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    Job j{c, nullptr, kp, false, n_sets, offsets, n_pairs, pair_q, pair_t, nullptr, idx, dist2, nullptr, nullptr, nullptr, err, errlen};
    j.desc8 = desc;
    j.is_u8 = true;
    return match_guarded(err, errlen, run, &j);
}

int sift_hip_match_u8(sift_hip_ctx* c, const uint8_t* desc, const sift_hip_keypoint* kp, int n_sets, const int64_t* offsets, int n_pairs,
                      const int32_t* pair_q, const int32_t* pair_t, const sift_hip_match_params* params, sift_hip_match_rec* recs,
                      int32_t* counts, int64_t* total, char* err, int errlen) {
    if (!c) { match_set_err(err, errlen, "sift_hip_match_u8: no context (matching runs on the GPU only)"); return SIFT_HIP_EINVAL; }
    if (!params) { match_set_err(err, errlen, "sift_hip_match_u8: no parameters"); return SIFT_HIP_EINVAL; }
    Job j{c, nullptr, kp, false, n_sets, offsets, n_pairs, pair_q, pair_t, params, nullptr, nullptr, recs, counts, total, err, errlen};
    j.desc8 = desc;
    j.is_u8 = true;
    return match_guarded(err, errlen, run, &j);
}

}  // extern "C"
