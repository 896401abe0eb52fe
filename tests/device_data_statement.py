"""The numpy statement of the device-resident voxel dataset (csrc/dataset.hip, include/pcd_hip.h): Philox4x32-10 in uint32 / uint64
numpy, the header's counter layout, the packing, the unaugmented arithmetic in fp32 operation by operation (the kernel must give the
same bits) and the augmented path in float64 (the kernel's fp32 must stay within rounding of it).  Shared by
tests/test_device_data_cpu.py and tests/test_gpu_device_data.py; nothing here imports the package."""
import numpy as np

WORDS = 1024
CTR_KEY, CTR_ANGLE, CTR_JITTER, CTR_DRAW, CTR_SPAN = 0, 8192, 16384, 65536, 1 << 24
KEY_COUNTERS, JITTER_COUNTERS = 8192, 32768          # 32768 keys at 4 a counter; one counter per point
NORMALIZE, ROTATE, JITTER = 1, 2, 4
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_words(counter, key) -> np.ndarray:
    """Philox4x32-10 proper: four counter words (each a uint64 array holding 32 bits) under the key words (k0, k1), the key bumped
    by (0x9E3779B9, 0xBB67AE85) after every round; (n, 4) uint32."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) for w in counter]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]                 # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=1).astype(np.uint32)


def philox4x32(ctr, seed: int) -> np.ndarray:
    """The library's use of it: 64-bit counters `ctr` as words {lo, hi, 0, 0}, 64-bit `seed` as key {lo(seed), hi(seed)}."""
    ctr = np.atleast_1d(np.asarray(ctr, dtype=np.uint64))
    zero = np.zeros_like(ctr)
    return philox4x32_words((ctr & M32, ctr >> np.uint64(32), zero, zero), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def span_ranges(num_points: int, slot: int, offset: int = 0) -> dict:
    """The half-open counter ranges slot `slot` may touch, by purpose, for clouds of up to 32768 voxels resampled to `num_points`."""
    base = offset + slot * CTR_SPAN
    return {"key": (base + CTR_KEY, base + CTR_KEY + KEY_COUNTERS), "angle": (base + CTR_ANGLE, base + CTR_ANGLE + 1),
            "jitter": (base + CTR_JITTER, base + CTR_JITTER + JITTER_COUNTERS),
            "draw": (base + CTR_DRAW, base + CTR_DRAW + (num_points + 3) // 4), "span": (base, base + CTR_SPAN)}


def pack(occupied: np.ndarray) -> np.ndarray:
    """(32, 32, 32) occupancy [z][y][x] -> 1024 uint32 words: word z * 32 + y, bit x."""
    occ = np.asarray(occupied, dtype=bool)
    words = np.zeros(WORDS, dtype=np.uint32)
    for z, y, x in zip(*np.nonzero(occ)):
        words[z * 32 + y] |= np.uint32(1) << np.uint32(x)
    return words


def unpack(words: np.ndarray) -> np.ndarray:
    out = np.zeros((32, 32, 32), dtype=bool)
    for w, v in enumerate(np.asarray(words, dtype=np.uint32)):
        for x in range(32):
            out[w >> 5, w & 31, x] = (int(v) >> x) & 1
    return out


def scan_points(words: np.ndarray) -> np.ndarray:
    """(M, 3) integer (z, y, x) of the set bits in ascending (word, bit): np.where's order on the unpacked grid."""
    return np.array(np.where(unpack(words))).T


def keys(m: int, seed: int, ctr0: int) -> np.ndarray:
    """The 32-bit subset key of every ordinal below m."""
    q = np.arange((m + 3) // 4, dtype=np.uint64) + np.uint64(ctr0 + CTR_KEY)
    return philox4x32(q, seed).reshape(-1)[:m]


def resample_ordinals(m: int, n: int, seed: int, ctr0: int) -> np.ndarray:
    """Which points (ordinals in scan order) make the n output rows."""
    if m == n:
        return np.arange(m)
    if m > n:
        k = keys(m, seed, ctr0)
        chosen = np.lexsort((np.arange(m), k))[:n]         # the n smallest (key, ordinal) pairs
        return np.sort(chosen)
    q = np.arange((n - m + 3) // 4, dtype=np.uint64) + np.uint64(ctr0 + CTR_DRAW)
    u = philox4x32(q, seed).reshape(-1)[:n - m].astype(np.uint64)
    return np.concatenate([np.arange(m), ((u * np.uint64(m)) >> np.uint64(32)).astype(np.int64)])


def normalize_fp32(p: np.ndarray):
    """`normalize_point_cloud` on integer points in fp32, operation by operation: exact integer column sums, mean = float(sum) /
    float(M), radius = sqrt(max((dz dz + dy dy) + dx dx)), (p - mean) / radius.  Returns (cloud, mean, radius)."""
    f = np.float32
    sums = p.astype(np.int64).sum(axis=0)
    assert sums.max() < 1 << 24
    mean = sums.astype(f) / f(len(p))
    d = p.astype(f) - mean
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    radius = np.sqrt(d2.max())                            # the correctly rounded root is monotonic: = max of the roots
    assert d.dtype == f and d2.dtype == f and radius.dtype == f
    return d / radius, mean, radius


def cloud_fp32(words: np.ndarray, n: int, seed: int, offset: int, slot: int, normalize: bool = True):
    """The unaugmented output rows of one slot, bit for bit, and M."""
    p = scan_points(words)
    m = len(p)
    if m == 0:
        return np.zeros((n, 3), np.float32), 0
    rows = resample_ordinals(m, n, seed, offset + slot * CTR_SPAN)
    cloud = normalize_fp32(p)[0] if normalize else p.astype(np.float32)
    return cloud[rows], m


def normals(m: int, seed: int, ctr0: int) -> np.ndarray:
    """(m, 3) float64: Box-Muller values 0, 1, 2 of counter JITTER + i for point i, from the 24-bit uniforms the device forms."""
    w = philox4x32(np.arange(m, dtype=np.uint64) + np.uint64(ctr0 + CTR_JITTER), seed)
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) / 16777216.0
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]), r1 * np.cos(2 * np.pi * u[:, 3])], axis=1)


def _normalize64(p):
    p = p - p.mean(axis=0)
    return p / np.sqrt((p ** 2).sum(axis=1)).max()


def cloud_f64(words: np.ndarray, n: int, seed: int, offset: int, slot: int, flags: int, sigma: float = 0.01, clip: float = 0.05):
    """The output rows of one slot in float64, augmentations in `PointCloudDataset._load`'s order."""
    p = scan_points(words).astype(np.float64)
    m = len(p)
    ctr0 = offset + slot * CTR_SPAN
    if flags & ROTATE:
        u = ((int(philox4x32(ctr0 + CTR_ANGLE, seed)[0, 0]) >> 8) + 0.5) / 16777216.0
        c, s = np.cos(2 * np.pi * u), np.sin(2 * np.pi * u)
        p = _normalize64(p) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    if flags & JITTER:
        p = p + np.clip(sigma * normals(m, seed, ctr0), -clip, clip)
    if flags & NORMALIZE:
        p = _normalize64(p)
    return p[resample_ordinals(m, n, seed, ctr0)], m


# ---------------------------------------------------------------------------------------------- shared test grids
def grid_with_count(m: int, seed: int) -> np.ndarray:
    """A 32^3 occupancy with exactly m voxels at random places."""
    occ = np.zeros(32 ** 3, dtype=bool)
    occ[np.random.default_rng(seed).permutation(32 ** 3)[:m]] = True
    return occ.reshape(32, 32, 32)


def ellipsoid_grid(seed: int, blobs: int = 3, rmin: float = 3, rmax: float = 9) -> np.ndarray:
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    c, r = rng.uniform(8, 24, (blobs, 3)), rng.uniform(rmin, rmax, (blobs, 3))
    occ = np.zeros((32, 32, 32), bool)
    for j in range(blobs):
        occ |= ((zz - c[j, 0]) / r[j, 0]) ** 2 + ((yy - c[j, 1]) / r[j, 1]) ** 2 + ((xx - c[j, 2]) / r[j, 2]) ** 2 <= 1
    return occ


def write_voxel_dir(root, count: int, seed: int = 5, synsets=("04379243", "03001627", "02691156")) -> list:
    """`count` ellipsoid grids as .npz files named like the reference's (synset id in the 5th '_' field); returns the names."""
    import os
    os.makedirs(root, exist_ok=True)
    names = []
    for i in range(count):
        name = f"vox_32_res_model_{synsets[i % len(synsets)]}_{i:03d}.npz"
        np.savez(os.path.join(root, name), data=ellipsoid_grid(seed * 1000 + i).astype(np.float32) * (1.0 + i % 3))
        names.append(name)
    return names
