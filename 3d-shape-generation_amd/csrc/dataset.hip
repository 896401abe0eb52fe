// Device-resident voxel dataset (include/pcd_hip.h: pcd_voxel_batch_clouds, pcd_voxel_batch_grids): bit-packed 32^3 grids -> a batch of point clouds
// (threshold is done at packing time; scan order, centroid, unit radius, resample to N) or of dense occupancy grids, one launch per batch.
//
// pcd_voxel_batch_clouds: one workgroup of 1024 lanes per batch slot, lane t owns word t = z * 32 + y of the slot's grid (bit x).  The ordinal of a point
// is its position in np.where's row-major order: base[t] (exclusive scan of the popcounts) + the rank of its bit in the word, so a lane walks a run of
// consecutive ordinals and ascending lanes walk ascending runs: a block scan over per-lane counts is an ordered compaction.  Nothing is kept per point:
// Philox keys, jitter normals and coordinates are recomputed in every pass that needs them (at M = 32768 a stored cloud would not fit the LDS).
#include "common.h"

namespace pcd {

constexpr int VOX_WORDS = 1024;                 // 32 * 32 words of 32 bits
constexpr int VOX_LANES = 1024;
constexpr int VOX_WAVES = VOX_LANES / 64;

struct VoxShared {
    uint32_t words[VOX_WORDS];
    uint32_t base[VOX_WORDS + 1];               // base[t]: ordinal of the first point of word t; base[1024] = M
    uint32_t hist[256];
    uint32_t wave_u[VOX_WAVES];
    float wave_f[VOX_WAVES];
    uint32_t pick[2];                           // radix select: the digit found and the rank left inside it
};

// the sum of one value per lane; safe to call back to back
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t* wave_u) {
    uint32_t total;
    block_scan_excl<VOX_WAVES>(v, wave_u, &total);
    return total;
}


// what a slot's run is made of, uniform over the workgroup
struct VoxSlot {                                // field for field mesh_data.hip's MdtSlot: the two chains are kept apart, see profiles/mesh_family_isa.md
    uint64_t seed, ctr0;                        // ctr0: first counter of the slot's span
    int flags;
    float sigma, clip;
    float mean0[3], rad0;                       // centroid and radius of the integer cloud (exact sums)
    float cs, sn;                               // rotation
    float mean1[3], rad1;                       // centroid and radius of the augmented cloud
};

#pragma clang fp contract(off)
// squared distance from m in the statement's order: (dz^2 + dy^2) + dx^2
__device__ __forceinline__ float dist2(const float (&p)[3], const float (&m)[3]) {
    const float a = p[0] - m[0], b = p[1] - m[1], c = p[2] - m[2];
    return (a * a + b * b) + c * c;
}

// point `ord` at integer (z, y, x) after rotation and jitter (PointCloudDataset._load, before its last normalisation)
__device__ __forceinline__ void augmented_point(const VoxSlot& s, uint32_t ord, int z, int y, int x, float (&p)[3]) {
    p[0] = (float)z; p[1] = (float)y; p[2] = (float)x;
    if (s.flags & PCD_VOXEL_ROTATE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = ((p[c] - s.mean0[c]) / s.rad0);
        const float p0 = p[0], p2 = p[2];
        p[0] = p0 * s.cs - p2 * s.sn;           // right-multiplication by [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        p[2] = p0 * s.sn + p2 * s.cs;
    }
    if (s.flags & PCD_VOXEL_JITTER) {
        float v[4];
        philox_normals4(s.ctr0 + PCD_VOXEL_CTR_JITTER + ord, s.seed, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] += fminf(fmaxf(s.sigma * v[c], -s.clip), s.clip);
    }
}

// the output row of point `ord`
__device__ __forceinline__ void emit_point(const VoxSlot& s, uint32_t ord, int z, int y, int x, float* __restrict__ row) {
    float p[3];
    if (s.flags & (PCD_VOXEL_ROTATE | PCD_VOXEL_JITTER)) {
        augmented_point(s, ord, z, y, x, p);
        if (s.flags & PCD_VOXEL_NORMALIZE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = ((p[c] - s.mean1[c]) / s.rad1);
        }
    } else {
        p[0] = (float)z; p[1] = (float)y; p[2] = (float)x;
        if (s.flags & PCD_VOXEL_NORMALIZE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = ((p[c] - s.mean0[c]) / s.rad0);
        }
    }
    row[0] = p[0]; row[1] = p[1]; row[2] = p[2];
}
#pragma clang fp contract(fast)

// x of the k-th (from 0) set bit of w; k < popcount(w)
__device__ __forceinline__ int kth_set_bit(uint32_t w, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i) w &= w - 1;
    return __builtin_ctz(w);
}

__global__ __launch_bounds__(VOX_LANES) void voxel_batch_clouds_kernel(const uint32_t* __restrict__ grids, int n_grids, const int* __restrict__ index,
                                                                         int n_points, uint64_t seed, uint64_t offset, int flags, float sigma, float clip,
                                                                         float* __restrict__ out, int* __restrict__ counts) {
    __shared__ VoxShared sh;
    const int t = threadIdx.x, b = blockIdx.x;
    const uint32_t N = (uint32_t)n_points;
    float* __restrict__ rows = out + (size_t)b * N * 3;
    const int g = index[b];
    if (g < 0 || g >= n_grids) {                 // uniform: an index outside the table reads nothing; zero rows, count -1
        for (size_t i = t; i < (size_t)N * 3; i += VOX_LANES) rows[i] = 0.f;
        if (t == 0) counts[b] = -1;
        return;
    }
    // ---------------------------------------------------------------- scan
    const uint32_t word = grids[(size_t)g * VOX_WORDS + t];
    const uint32_t cnt = (uint32_t)__builtin_popcount(word);
    const int z = t >> 5, y = t & 31;
    uint32_t M;
    const uint32_t base = block_scan_excl<VOX_WAVES>(cnt, sh.wave_u, &M);
    sh.words[t] = word;
    sh.base[t] = base;
    if (t == 0) { sh.base[VOX_WORDS] = M; counts[b] = (int)M; }
    if (M == 0) {                                // uniform
        for (size_t i = t; i < (size_t)N * 3; i += VOX_LANES) rows[i] = 0.f;
        return;
    }
    VoxSlot s;
    s.seed = seed; s.ctr0 = offset + (uint64_t)b * PCD_VOXEL_CTR_SPAN; s.flags = flags; s.sigma = sigma; s.clip = clip;
    s.rad0 = s.rad1 = 1.f; s.cs = 1.f; s.sn = 0.f;
    for (int c = 0; c < 3; ++c) s.mean0[c] = s.mean1[c] = 0.f;
    const bool augmented = (flags & (PCD_VOXEL_ROTATE | PCD_VOXEL_JITTER)) != 0;
    // ---------------------------------------------------------------- centroid and radius of the integer cloud
    if ((flags & PCD_VOXEL_ROTATE) || ((flags & PCD_VOXEL_NORMALIZE) && !augmented)) {
        uint32_t sx = 0;
        for (uint32_t w = word; w; w &= w - 1) sx += (uint32_t)__builtin_ctz(w);
        const uint32_t sum_z = block_sum_u32(cnt * (uint32_t)z, sh.wave_u);      // <= 31 * 32768 < 2^24: exact in fp32
        const uint32_t sum_y = block_sum_u32(cnt * (uint32_t)y, sh.wave_u);
        const uint32_t sum_x = block_sum_u32(sx, sh.wave_u);
        const float fm = (float)M;
        s.mean0[0] = ((float)sum_z) / fm;
        s.mean0[1] = ((float)sum_y) / fm;
        s.mean0[2] = ((float)sum_x) / fm;
        float d2 = 0.f;
        for (uint32_t w = word; w; w &= w - 1) {
            const float p[3] = {(float)z, (float)y, (float)__builtin_ctz(w)};
            d2 = fmaxf(d2, dist2(p, s.mean0));
        }
        d2 = block_reduce(d2, MaxOp(), sh.wave_f);
        s.rad0 = sqrtf(d2);                 // the correctly rounded root is monotonic: max of the roots = root of the max
    }
    if (flags & PCD_VOXEL_ROTATE) {
        uint32_t c[4];
        philox_words4(s.ctr0 + PCD_VOXEL_CTR_ANGLE, seed, c);
        const float u = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        sincosf(6.28318530717958647692f * u, &s.sn, &s.cs);
    }
    // ---------------------------------------------------------------- centroid and radius of the augmented cloud: float sums in a fixed order
    if (augmented && (flags & PCD_VOXEL_NORMALIZE)) {
        float acc[3] = {0.f, 0.f, 0.f};
        uint32_t ord = base;
        for (uint32_t w = word; w; w &= w - 1, ++ord) {
            float p[3];
            augmented_point(s, ord, z, y, __builtin_ctz(w), p);
            acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2];
        }
        for (int c = 0; c < 3; ++c) s.mean1[c] = (block_reduce(acc[c], SumOp(), sh.wave_f)) / (float)M;
        float d2 = 0.f;
        ord = base;
        for (uint32_t w = word; w; w &= w - 1, ++ord) {
            float p[3];
            augmented_point(s, ord, z, y, __builtin_ctz(w), p);
            d2 = fmaxf(d2, dist2(p, s.mean1));
        }
        s.rad1 = sqrtf(block_reduce(d2, MaxOp(), sh.wave_f));
    }
    __syncthreads();                              // words / base visible; the reductions' scratch is free
    // ---------------------------------------------------------------- resample
    if (M <= N) {
        uint32_t ord = base;
        for (uint32_t w = word; w; w &= w - 1, ++ord) emit_point(s, ord, z, y, __builtin_ctz(w), rows + (size_t)ord * 3);
        // N - M draws with replacement, draw j = word j & 3 of counter DRAW + (j >> 2), ordinal = mulhi(u, M)
        const uint32_t draws = N - M;
        for (uint32_t q = t; q * 4 < draws; q += VOX_LANES) {
            uint32_t c[4];
            philox_words4(s.ctr0 + PCD_VOXEL_CTR_DRAW + q, seed, c);
            for (int e = 0; e < 4; ++e) {
                const uint32_t j = q * 4 + e;
                if (j >= draws) break;
                const uint32_t o = __umulhi(c[e], M);
                int lo = 0, hi = VOX_WORDS;      // the last word with base <= o: base[lo] <= o < base[hi] throughout (base[0] = 0, base[1024] = M > o)
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (sh.base[mid] <= o) lo = mid; else hi = mid;
                }
                const int x = kth_set_bit(sh.words[lo], o - sh.base[lo]);
                emit_point(s, o, lo >> 5, lo & 31, x, rows + (size_t)(M + j) * 3);
            }
        }
        return;
    }
    // M > N: the N smallest (key, ordinal) pairs; key of ordinal i = word i & 3 of counter KEY + (i >> 2).  Radix select of the N-th smallest key,
    // most significant byte first: `prefix` holds the bytes found, `rank` the 1-based rank still looked for among the keys that share them.
    uint32_t prefix = 0, rank = N;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (t < 256) sh.hist[t] = 0;
        __syncthreads();
        for (uint32_t q = t; q * 4 < M; q += VOX_LANES) {
            uint32_t c[4];
            philox_words4(s.ctr0 + PCD_VOXEL_CTR_KEY + q, seed, c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool live = q * 4 + e < M && (pass == 0 || (c[e] >> (shift + 8)) == prefix);
                if (live) atomicAdd(&sh.hist[(c[e] >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        const uint32_t h = t < 256 ? sh.hist[t] : 0u;
        const uint32_t before = block_scan_excl<VOX_WAVES>(h, sh.wave_u);
        if (t < 256 && before < rank && rank <= before + h) { sh.pick[0] = (uint32_t)t; sh.pick[1] = rank - before; }
        __syncthreads();
        prefix = (prefix << 8) | sh.pick[0];
        rank = sh.pick[1];
        __syncthreads();
    }
    // keys below `prefix` are all in, and the first `rank` ordinals whose key equals it.  Ordered compaction: rows ascend with the ordinal.
    const uint32_t cut = prefix, ties = rank;
    uint32_t below = 0, equal = 0;               // one bit per point of this word, in the order of its set bits
    {
        uint32_t c[4] = {0, 0, 0, 0};
        uint32_t ord = base, have = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < cnt; ++i, ++ord) {
            if ((ord >> 2) != have) { have = ord >> 2; philox_words4(s.ctr0 + PCD_VOXEL_CTR_KEY + have, seed, c); }
            const uint32_t e = ord & 3u;
            const uint32_t key = e == 0 ? c[0] : e == 1 ? c[1] : e == 2 ? c[2] : c[3];
            below |= (uint32_t)(key < cut) << i;
            equal |= (uint32_t)(key == cut) << i;
        }
    }
    const uint32_t nb = (uint32_t)__builtin_popcount(below), ne = (uint32_t)__builtin_popcount(equal);
    uint32_t b_before = block_scan_excl<VOX_WAVES>(nb, sh.wave_u);
    uint32_t e_before = block_scan_excl<VOX_WAVES>(ne, sh.wave_u);
    uint32_t ord = base, i = 0;
    for (uint32_t w = word; w; w &= w - 1, ++ord, ++i) {
        const bool is_b = (below >> i) & 1u, is_e = (equal >> i) & 1u;
        if (is_b || (is_e && e_before < ties)) {
            const uint32_t row = b_before + (e_before < ties ? e_before : ties);
            if (row < N) emit_point(s, ord, z, y, __builtin_ctz(w), rows + (size_t)row * 3);
        }
        b_before += is_b;
        e_before += is_e;
    }
}

// out[b][0][z][y][x] = bit x of word z * 32 + y: four consecutive x per lane
__global__ __launch_bounds__(256) void voxel_batch_grids_kernel(const uint32_t* __restrict__ grids, int n_grids, const int* __restrict__ index,
                                                                  int64_t quads, float* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= quads) return;
    const int b = (int)(q >> 13), in = (int)(q & 8191);          // 8192 quads per grid
    const int g = index[b];
    const uint32_t w = (g >= 0 && g < n_grids) ? grids[(size_t)g * VOX_WORDS + (in >> 3)] : 0u;
    const uint32_t nib = (w >> ((in & 7) * 4)) & 15u;
    f32x4 v;
    v[0] = (float)(nib & 1u); v[1] = (float)((nib >> 1) & 1u); v[2] = (float)((nib >> 2) & 1u); v[3] = (float)((nib >> 3) & 1u);
    *reinterpret_cast<f32x4*>(out + q * 4) = v;
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_voxel_batch_clouds(const uint32_t* grids, int n_grids, const int* index, int batch, int num_points, uint64_t seed,
                                      uint64_t offset, int flags, float sigma, float clip, float* out, int* counts, void* stream) {
    PCD_CHECK_ARG(grids && index && out && counts);
    PCD_CHECK_ARG(n_grids > 0 && batch > 0 && num_points > 0 && num_points <= PCD_VOXEL_MAX_POINTS);
    PCD_CHECK_ARG((flags & ~(PCD_VOXEL_NORMALIZE | PCD_VOXEL_ROTATE | PCD_VOXEL_JITTER)) == 0);
    hipLaunchKernelGGL(voxel_batch_clouds_kernel, dim3(batch), dim3(VOX_LANES), 0, (hipStream_t)stream, grids, n_grids, index, num_points, seed,
                       offset, flags, sigma, clip, out, counts);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_voxel_batch_grids(const uint32_t* grids, int n_grids, const int* index, int batch, float* out, void* stream) {
    PCD_CHECK_ARG(grids && index && out && n_grids > 0 && batch > 0);
    const int64_t quads = (int64_t)batch * 8192;
    hipLaunchKernelGGL(voxel_batch_grids_kernel, dim3((unsigned)ceil_div(quads, 256)), dim3(256), 0, (hipStream_t)stream, grids, n_grids, index,
                       quads, out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
