"""Data layer feeding the samplers and the evaluation scripts (reference data.py:11-371).

Host-side numpy, like the reference: voxel grid file -> min-max normalised occupancy -> (optionally) point
cloud of voxel coordinates -> centroid-centred, unit-radius cloud -> resampled to `num_points`.  The class and
method names, constructor arguments and defaults follow the reference so its entry scripts read the same.

Differences, both deliberate:
  * no Lightning: `PointCloudDataModule` / `PointCloudDataDirectoryModule` are plain objects with the same
    `setup()` / `train_dataloader()` / `val_dataloader()` surface;
  * `DeviceVoxelDataModule` (not in the reference): the same directory read once, the grids bit-packed on the GPU and each batch
    assembled by one kernel launch (csrc/dataset.hip); opt-in, the host modules are unchanged;
  * `DeviceMeshDataModule` (not in the reference): triangle meshes resident on the GPU, every batch freshly drawn from their surfaces
    by one kernel launch (csrc/mesh_data.hip); labels from the subdirectories;
  * file format: the reference stores each sample as a deepdish HDF5 file `*.dd` read with
    `dd.io.load(path)['data']` (data.py:176).  deepdish/h5py are not part of this image, so besides `.dd`
    (read through h5py when it is importable) the dataset accepts `.npz` (key `data`) and `.npy` files with
    the same naming scheme; `convert_dd_to_npz` rewrites a directory once on a machine that has h5py.
"""
from __future__ import annotations

import os
import random
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, TensorDataset

_EXTS = (".dd", ".npz", ".npy")

# ShapeNet synset id -> category name (reference data.py:82-138); the id is the 5th '_' field of a file name
SHAPENET_ID_TO_CATEGORY = {
    "02691156": "airplane", "02747177": "ashcan", "02773838": "bag", "02801938": "basket", "02808440": "bathtub",
    "02818832": "bed", "02828884": "bench", "02843684": "birdhouse", "02871439": "bookshelf", "02876657": "bottle",
    "02880940": "bowl", "02924116": "bus", "02933112": "cabinet", "02942699": "camera", "02946921": "can",
    "02954340": "cap", "02958343": "car", "02992529": "cellular_telephone", "03001627": "chair", "03046257": "clock",
    "03085013": "computer_keyboard", "03207941": "dishwasher", "03211117": "display", "03261776": "earphone",
    "03325088": "faucet", "03337140": "file", "03467517": "guitar", "03513137": "helmet", "03593526": "jar",
    "03624134": "knife", "03636649": "lamp", "03642806": "laptop", "03691459": "loudspeaker", "03710193": "mailbox",
    "03759954": "microphone", "03761084": "microwave", "03790512": "motorcycle", "03797390": "mug", "03928116": "piano",
    "03938244": "pillow", "03948459": "pistol", "03991062": "pot", "04004475": "printer", "04074963": "remote_control",
    "04090263": "rifle", "04099429": "rocket", "04225987": "skateboard", "04256520": "sofa", "04330267": "stove",
    "04379243": "table", "04401088": "telephone", "04460130": "tower", "04468005": "train", "04530566": "vessel",
    "04554684": "washer",
}


def load_sample_file(path: str) -> np.ndarray:
    """The `data` array of one sample file (reference: `dd.io.load(file_path)['data']`, data.py:176,192)."""
    if path.endswith(".npz"):
        with np.load(path) as f:
            return f["data"]
    if path.endswith(".npy"):
        return np.load(path)
    if path.endswith(".dd"):
        try:
            import h5py
        except ImportError as e:
            raise RuntimeError(f"{path}: reading deepdish .dd files needs h5py, which is not installed here; convert "
                               "the directory once with shapegen_amd.data.convert_dd_to_npz on a machine that has it") from e
        with h5py.File(path, "r") as f:
            return np.asarray(f["data"])
    raise ValueError(f"unsupported sample file {path}")


def convert_dd_to_npz(src_dir: str, dst_dir: str) -> int:
    """Rewrite every `*.dd` under src_dir as `<same name>.npz` (key `data`) in dst_dir; returns the count."""
    os.makedirs(dst_dir, exist_ok=True)
    n = 0
    for f in sorted(os.listdir(src_dir)):
        if f.endswith(".dd"):
            np.savez_compressed(os.path.join(dst_dir, f[:-3] + ".npz"), data=load_sample_file(os.path.join(src_dir, f)))
            n += 1
    return n


class PointCloudDataModule:
    """reference data.py:11-46: in-memory clouds -> random 80/20 split -> loaders.  With `labels` (one integer per cloud,
    not in the reference) an item is (cloud, int64 label)."""

    def __init__(self, point_clouds, batch_size=32, train_val_split=0.8, labels=None):
        self.point_clouds, self.batch_size, self.train_val_split = point_clouds, batch_size, train_val_split
        self.labels = labels
        if labels is not None and len(labels) != len(point_clouds):
            raise ValueError(f"{len(labels)} labels for {len(point_clouds)} clouds")

    def setup(self, stage=None):
        tensors = [torch.FloatTensor(np.asarray(self.point_clouds))]
        if self.labels is not None:
            tensors.append(torch.as_tensor(np.asarray(self.labels), dtype=torch.int64))
        dataset = TensorDataset(*tensors)
        train_size = int(self.train_val_split * len(dataset))
        self.train_dataset, self.val_dataset = torch.utils.data.random_split(dataset, [train_size, len(dataset) - train_size])

    def train_dataloader(self):
        return DataLoader(self.train_dataset, batch_size=self.batch_size, shuffle=True)

    def val_dataloader(self):
        return DataLoader(self.val_dataset, batch_size=self.batch_size)


class PointCloudDataset(Dataset):
    """reference data.py:48-311.  Returns a float32 tensor: (1,R,R,R) in 'voxels' output mode, (num_points,3)
    in 'point_clouds' output mode.  `return_labels` (not in the reference; voxel file mode only): an item is (tensor, int64
    label), the label being the index of the file's category in `categories`, the sorted distinct categories after filtering."""

    def __init__(self, data_dir, num_points=2048, transform=None, input_mode="voxels", output_mode="voxels",
                 normalize=True, jitter=True, rotate=False, resolution=32, relevant_object_categories=None, return_labels=False):
        self.data_dir = data_dir
        self.transform = transform
        self.num_points = num_points
        self.file_list: List[str] = [f for f in os.listdir(data_dir) if f.endswith(_EXTS)]
        self.input_mode = input_mode
        self.output_mode = output_mode
        self.normalize = normalize
        self.jitter = jitter
        self.rotate = rotate
        self.resolution = 32          # the reference ignores its `resolution` argument too (data.py:75)
        self.relevant_object_categories = ["all"] if relevant_object_categories is None else relevant_object_categories
        self.shapenet_id_to_category = SHAPENET_ID_TO_CATEGORY
        self.filter_file_list()
        self.return_labels = bool(return_labels)
        self.categories: List[str] = []
        if self.return_labels:
            if input_mode != "voxels":
                raise ValueError("return_labels needs input_mode='voxels': only those file names carry the ShapeNet synset id")
            self.categories = sorted({self.category_of(f) for f in self.file_list})

    def category_of(self, file_name: str) -> str:
        """The ShapeNet category of a voxel file (its synset id is the 5th '_' field of the name)."""
        return self.shapenet_id_to_category[file_name.split("_")[4]]

    def filter_file_list(self):
        """data.py:140-152: keep files whose synset id (5th '_' field) maps to a requested category."""
        if self.input_mode != "voxels" or self.relevant_object_categories == ["all"]:
            return
        self.file_list = [f for f in self.file_list
                          if self.shapenet_id_to_category[f.split("_")[4]] in self.relevant_object_categories]

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, idx):
        item = self._load(idx)
        if self.return_labels:
            return item, torch.tensor(self.categories.index(self.category_of(self.file_list[idx])), dtype=torch.int64)
        return item

    def _load(self, idx):
        file_path = os.path.join(self.data_dir, self.file_list[idx])
        if self.input_mode == "voxels":
            voxels = load_sample_file(file_path)
            self.resolution = voxels.shape[0]
            lo, hi = np.min(voxels), np.max(voxels)
            voxels = np.full_like(voxels, lo) if lo == hi else (voxels - lo) / (hi - lo)
            if self.output_mode == "voxels" and self.transform is None and not any([self.jitter, self.rotate]):
                return torch.FloatTensor(np.expand_dims(voxels, axis=0))
            point_cloud = self.voxel_to_point_cloud(voxels)
        elif self.input_mode == "point_clouds":
            point_cloud = load_sample_file(file_path)
        else:
            raise ValueError("Invalid input_mode for PointCloudDataset")

        if self.transform:
            point_cloud = self.transform(point_cloud)
        if self.rotate:
            point_cloud = self.rotate_around_vertical_axis(self.normalize_point_cloud(point_cloud))
        if self.jitter:
            point_cloud = self.jitter_points(point_cloud)

        if self.output_mode == "voxels":
            output = np.expand_dims(self.point_cloud_to_voxel(point_cloud, self.resolution), axis=0)
        elif self.output_mode == "point_clouds":
            if self.normalize:
                point_cloud = self.normalize_point_cloud(point_cloud)
            output = self.sample_point_cloud(point_cloud, self.num_points)
        else:
            raise ValueError("Invalid output_mode for PointCloudDataset")
        return torch.FloatTensor(output)

    # ------------------------------------------------------------------ deterministic pieces
    @staticmethod
    def voxel_to_point_cloud(voxels, threshold=0.5):
        """data.py:213-218: integer (z,y,x) indices of the occupied voxels, row-major scan order."""
        return np.array(np.where(voxels > threshold)).T

    @staticmethod
    def point_cloud_to_voxel(point_cloud, resolution):
        """data.py:220-228: [-1,1] coordinates -> occupancy, written as grid[z,y,x] from columns (x,y,z)."""
        top = resolution - 1
        cell = np.clip((point_cloud + 1) * top / 2, 0, top).astype(int)          # truncation, after the clip, as the reference does
        x, y, z = cell[:, 0], cell[:, 1], cell[:, 2]
        grid = np.zeros((resolution,) * 3, dtype=np.float32)
        grid[z, y, x] = 1
        return grid

    @staticmethod
    def normalize_point_cloud(point_cloud):
        """data.py:230-238: subtract the centroid, divide by the largest distance from it."""
        point_cloud = point_cloud - np.mean(point_cloud, axis=0)
        return point_cloud / np.max(np.sqrt(np.sum(point_cloud ** 2, axis=1)))

    # ------------------------------------------------------------------ random pieces (python / numpy global RNGs)
    @staticmethod
    def sample_point_cloud(point_cloud, num_points):
        """data.py:240-254: exact size -> unchanged; more -> without replacement (`random.sample`); fewer -> every
        point once, then `np.random.choice` with replacement for the rest."""
        if len(point_cloud) == num_points:
            return point_cloud
        if len(point_cloud) > num_points:
            return point_cloud[random.sample(range(len(point_cloud)), num_points)]
        extra = np.random.choice(len(point_cloud), num_points - len(point_cloud), replace=True)
        return point_cloud[list(range(len(point_cloud))) + extra.tolist()]

    @staticmethod
    def farthest_point_sample(point_cloud, num_points):
        """data.py:256-287 (the reference's own pipeline does not call it: "makes dataloading very slow"): greedy farthest-point subset, first
        point from `np.random.randint`.  `nearest` = squared distance of every point to the subset so far (starts at 1e10)."""
        n = len(point_cloud)
        if n == num_points:
            return point_cloud
        xyz = point_cloud[:, :3]
        nearest = np.full((n,), 1e10)
        chosen = np.empty((num_points,), np.int32)
        nxt = np.random.randint(0, n)
        for k in range(num_points):
            chosen[k] = nxt
            np.minimum(nearest, np.sum((xyz - xyz[nxt, :]) ** 2, axis=-1), out=nearest)
            nxt = np.argmax(nearest, axis=-1)
        return point_cloud[chosen]

    @staticmethod
    def jitter_points(points, sigma=0.01, clip=0.05):
        """data.py:289-295."""
        return np.clip(sigma * np.random.randn(*points.shape), -clip, clip) + points

    @staticmethod
    def rotate_around_vertical_axis(point_cloud):
        """data.py:297-309: right-multiply by a rotation about the y axis by a uniform angle."""
        a = np.random.uniform() * 2 * np.pi
        c, s = np.cos(a), np.sin(a)
        return np.dot(point_cloud, np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]))


class PointCloudDataDirectoryModule:
    """reference data.py:311-371 (`augmentations=False` switches jitter and rotation off)."""

    def __init__(self, data_dir, num_points=2048, batch_size=32, num_workers=4, train_val_split=0.8,
                 file_mode="voxels", output_mode="point_clouds", augmentations=True, normalization=True,
                 relevant_object_categories: Optional[Sequence[str]] = None, return_labels=False):
        self.return_labels = return_labels
        self.data_dir, self.num_points, self.batch_size, self.num_workers = data_dir, num_points, batch_size, num_workers
        self.train_val_split, self.file_mode, self.output_mode = train_val_split, file_mode, output_mode
        self.augmentations, self.normalization = augmentations, normalization
        self.relevant_object_categories = relevant_object_categories

    def setup(self, stage=None):
        kw = dict(num_points=self.num_points, input_mode=self.file_mode, output_mode=self.output_mode,
                  normalize=self.normalization, relevant_object_categories=self.relevant_object_categories)
        if not self.augmentations:
            kw.update(rotate=False, jitter=False)
        if self.return_labels:
            kw.update(return_labels=True)
        full = PointCloudDataset(self.data_dir, **kw)
        self.categories = full.categories
        train_size = int(self.train_val_split * len(full))
        self.train_dataset, self.val_dataset = torch.utils.data.random_split(full, [train_size, len(full) - train_size])

    def train_dataloader(self):
        return DataLoader(self.train_dataset, batch_size=self.batch_size, shuffle=True, num_workers=self.num_workers)

    def val_dataloader(self):
        return DataLoader(self.val_dataset, batch_size=self.batch_size, num_workers=self.num_workers)


# ---------------------------------------------------------------------------------------------- device-resident voxel data
VOXEL_WORDS = 1024                       # a 32^3 grid as 32-bit words: word z * 32 + y, bit x (include/pcd_hip.h)
VOXEL_CTR_SPAN = 1 << 24                 # Philox counters owned by one batch slot (PCD_VOXEL_CTR_SPAN)
VOXEL_NORMALIZE, VOXEL_ROTATE, VOXEL_JITTER = 1, 2, 4
VAL_KEY = 0x5EED                         # the validation loader's fixed Philox key


def minmax_grid(voxels: np.ndarray) -> np.ndarray:
    """`PointCloudDataset._load`'s min-max normalisation of one grid, its `lo == hi` case included."""
    lo, hi = np.min(voxels), np.max(voxels)
    return np.full_like(voxels, lo) if lo == hi else (voxels - lo) / (hi - lo)


def pack_grids(occupied: np.ndarray) -> np.ndarray:
    """(S, 32, 32, 32) boolean occupancy [z][y][x] -> (S, 1024) uint32, word z * 32 + y, bit x."""
    occ = np.asarray(occupied, dtype=bool).reshape(-1, VOXEL_WORDS, 32)
    return np.packbits(occ, axis=2, bitorder="little").view("<u4").reshape(-1, VOXEL_WORDS).astype(np.uint32, copy=False)


def unpack_grids(packed: np.ndarray) -> np.ndarray:
    """Inverse of `pack_grids`: (S, 1024) uint32 -> (S, 32, 32, 32) bool."""
    w = np.asarray(packed, dtype=np.uint32).reshape(-1, VOXEL_WORDS, 1)
    return ((w >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1, 32, 32, 32)


class _Rows(Dataset):
    """The dataset `random_split` sees: row numbers of the packed table."""

    def __init__(self, count: int):
        self.count = count

    def __len__(self):
        return self.count

    def __getitem__(self, idx):
        return idx


class _DeviceLoader:
    """One pass over `rows` in batches, every batch one kernel launch.  Shuffled: the permutation and a 63-bit Philox key are drawn from
    the global torch generator when the iteration starts (where DataLoader's RandomSampler draws its seed)."""

    def __init__(self, module, rows: Sequence[int], shuffle: bool, ctr_span: int = VOXEL_CTR_SPAN):
        self.module, self.rows, self.shuffle = module, torch.as_tensor(list(rows), dtype=torch.int64), shuffle
        self.ctr_span = ctr_span             # Philox counters one batch slot owns in the module's kernel

    def __len__(self):
        return (len(self.rows) + self.module.batch_size - 1) // self.module.batch_size

    def __iter__(self):
        m, rows, key = self.module, self.rows, VAL_KEY
        if self.shuffle:
            rows = rows[torch.randperm(len(rows))]
            key = int(torch.empty((), dtype=torch.int64).random_().item())
        rows = rows.to(m.device)
        rows32 = rows.to(torch.int32)
        for i, lo in enumerate(range(0, len(rows), m.batch_size)):
            item = m.batch(rows32[lo:lo + m.batch_size], seed=key, offset=i * m.batch_size * self.ctr_span)
            if m.return_labels:
                labels = m.labels_device[rows[lo:lo + m.batch_size]]
                item = (*item, labels) if isinstance(item, tuple) else (item, labels)
            yield item


class DeviceVoxelDataModule:
    """`PointCloudDataDirectoryModule` for voxel files with the data resident on the GPU: `setup()` reads every file once, applies the
    dataset's min-max and `> 0.5` threshold, packs each 32^3 grid into 1024 words and uploads the table (4 KB a shape); a batch is one
    launch of `pcd_voxel_batch_clouds` (scan order -> centroid -> unit radius -> resample; `augmentations` adds the dataset's jitter
    before the normalisation, as the host module does, which never rotates; `rotate=True`, not an argument of the host module, adds the
    dataset's `rotate_around_vertical_axis` in front of it) or, in `output_mode="voxels"`, of `pcd_voxel_batch_grids`.  The split, the labels and `categories` are those of the
    host module under the same seed.  Two deliberate differences from the host path: the random draws are Philox streams keyed per epoch
    from the global torch generator (not python's / numpy's generators), and a subset of a cloud with more than `num_points` voxels comes
    out in scan order (the host's `random.sample` order is random).
    `grids=` (S, 32, 32, 32) with optional integer `labels=` replaces `data_dir` (tests, synthetic runs); `device="cpu"` keeps the packed
    table on the host, where `setup()` works and the loaders do not."""

    def __init__(self, data_dir=None, num_points=2048, batch_size=32, num_workers=4, train_val_split=0.8,
                 file_mode="voxels", output_mode="point_clouds", augmentations=True, normalization=True,
                 relevant_object_categories: Optional[Sequence[str]] = None, return_labels=False, device="cuda",
                 grids=None, labels=None, rotate=False, jitter_sigma=0.01, jitter_clip=0.05):
        if file_mode != "voxels":
            raise ValueError("DeviceVoxelDataModule reads voxel files only (file_mode='voxels')")
        if output_mode not in ("point_clouds", "voxels"):
            raise ValueError("Invalid output_mode for DeviceVoxelDataModule")
        if (data_dir is None) == (grids is None):
            raise ValueError("give either data_dir or grids")
        if output_mode == "voxels" and (augmentations or rotate):
            raise ValueError("output_mode='voxels' is served without augmentations only (pass augmentations=False)")
        if return_labels and grids is not None and labels is None:
            raise ValueError("return_labels with grids= needs labels=")
        self.return_labels = return_labels
        self.data_dir, self.num_points, self.batch_size, self.num_workers = data_dir, num_points, batch_size, num_workers
        self.train_val_split, self.file_mode, self.output_mode = train_val_split, file_mode, output_mode
        self.augmentations, self.normalization = augmentations, normalization
        self.relevant_object_categories = relevant_object_categories
        self.device, self.grids, self.labels = torch.device(device), grids, labels
        self.jitter_sigma, self.jitter_clip = float(jitter_sigma), float(jitter_clip)
        # PointCloudDataDirectoryModule switches jitter and rotation off without `augmentations` and otherwise leaves the dataset's
        # defaults, jitter=True, rotate=False: `augmentations` means jitter
        self.rotate = bool(rotate)
        self.flags = ((VOXEL_NORMALIZE if normalization else 0) | (VOXEL_JITTER if augmentations else 0)
                      | (VOXEL_ROTATE if rotate else 0))
        self._counts = None
        self.categories: List[str] = []

    def _occupancy(self, voxels: np.ndarray, name: str) -> np.ndarray:
        voxels = np.asarray(voxels)
        if voxels.shape != (32, 32, 32):
            raise ValueError(f"{name}: the grid is {tuple(voxels.shape)}, not (32, 32, 32)")
        v = minmax_grid(voxels)
        occ = v > 0.5
        if self.output_mode == "voxels" and not np.all((v == 0) | (v == 1)):
            raise ValueError(f"{name}: the grid is not binary after min-max normalisation; the packed table holds occupancy bits only")
        if int(occ.sum()) < 2:
            raise ValueError(f"{name}: {int(occ.sum())} occupied voxels; a point cloud needs at least 2 (its radius would be zero)")
        return occ

    def setup(self, stage=None):
        if self.grids is not None:
            names = [f"grids[{i}]" for i in range(len(self.grids))]
            raw = self.grids
            labels = None if self.labels is None else [int(v) for v in self.labels]
            if labels is not None and len(labels) != len(names):
                raise ValueError(f"{len(labels)} labels for {len(names)} grids")
        else:
            # the host dataset lists, filters and labels the files: same order, same categories
            full = PointCloudDataset(self.data_dir, num_points=self.num_points, input_mode="voxels", output_mode=self.output_mode,
                                     relevant_object_categories=self.relevant_object_categories, return_labels=self.return_labels)
            self.file_list, self.categories = full.file_list, full.categories
            names = [os.path.join(self.data_dir, f) for f in full.file_list]
            raw = (load_sample_file(p) for p in names)
            labels = [full.categories.index(full.category_of(f)) for f in full.file_list] if self.return_labels else None
        self.packed_host = np.zeros((len(names), VOXEL_WORDS), dtype=np.uint32)      # packed grid by grid: 4 KB a shape on the host too
        self.counts = np.zeros(len(names), dtype=np.int64)
        for i, (name, voxels) in enumerate(zip(names, raw)):
            occ = self._occupancy(voxels, name)
            self.packed_host[i], self.counts[i] = pack_grids(occ)[0], occ.sum()
        self.packed = torch.from_numpy(self.packed_host.view(np.int32)).to(self.device)
        self.labels_device = None if labels is None else torch.as_tensor(labels, dtype=torch.int64, device=self.device)
        rows = _Rows(len(names))
        train_size = int(self.train_val_split * len(rows))
        self.train_dataset, self.val_dataset = torch.utils.data.random_split(rows, [train_size, len(rows) - train_size])

    def batch(self, index: torch.Tensor, seed: int, offset: int) -> torch.Tensor:
        """The batch of the packed rows `index` (device int32) under Philox key `seed`, slot b's counters starting at
        `offset + b * VOXEL_CTR_SPAN`: (B, num_points, 3) clouds, or (B, 1, 32, 32, 32) grids in voxel mode."""
        from . import _lib
        if self.packed.device.type != "cuda":
            raise RuntimeError("DeviceVoxelDataModule assembles batches on the GPU: construct it with device='cuda' (no CPU path)")
        lib, b = _lib.load(), int(index.numel())
        if self.output_mode == "voxels":
            out = torch.empty((b, 1, 32, 32, 32), dtype=torch.float32, device=self.packed.device)
            _lib.check(lib.pcd_voxel_batch_grids(_lib.ptr(self.packed), self.packed.shape[0], _lib.ptr(index), b, _lib.ptr(out),
                                                 _lib.stream_ptr()), "voxel_batch_grids")
            return out
        out = torch.empty((b, self.num_points, 3), dtype=torch.float32, device=self.packed.device)
        if self._counts is None or self._counts.numel() < b:                         # the kernel's M per slot; one buffer per module
            self._counts = torch.empty((max(b, self.batch_size),), dtype=torch.int32, device=self.packed.device)
        _lib.check(lib.pcd_voxel_batch_clouds(_lib.ptr(self.packed), self.packed.shape[0], _lib.ptr(index), b, self.num_points,
                                              seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF, self.flags, self.jitter_sigma,
                                              self.jitter_clip, _lib.ptr(out), _lib.ptr(self._counts), _lib.stream_ptr()), "voxel_batch_clouds")
        return out

    def train_dataloader(self):
        return _DeviceLoader(self, self.train_dataset.indices, shuffle=True)

    def val_dataloader(self):
        return _DeviceLoader(self, self.val_dataset.indices, shuffle=False)


# ---------------------------------------------------------------------------------------------- device-resident mesh data
MESH_CTR_SPAN = 1 << 26                  # Philox counters owned by one batch slot (PCD_MESH_CTR_SPAN)
MESH_MAX_POINTS = 1 << 24                # PCD_MESH_MAX_POINTS
_MESH_EXTS = (".obj", ".ply")


def mesh_files(data_dir: str) -> List[str]:
    """The `.obj` / `.ply` files under `data_dir`, as paths relative to it, sorted."""
    found = []
    for root, _, files in os.walk(data_dir):
        found += [os.path.relpath(os.path.join(root, f), data_dir) for f in files if f.lower().endswith(_MESH_EXTS)]
    return sorted(found)


def mesh_category(relative_path: str) -> str:
    """The category of a mesh file: the subdirectory of the data directory that holds it, "" for a file directly in it."""
    parts = relative_path.split(os.sep)
    return parts[0] if len(parts) > 1 else ""


class DeviceMeshDataModule:
    """Triangle meshes resident on the GPU, every batch a fresh draw from their surfaces: `setup()` reads every `.obj` / `.ply` file under
    `data_dir` once (`utils.load_mesh`, sorted order), packs them into one table -- vertices, faces local to the mesh, offsets -- uploads
    it and runs `pcd_mesh_area_sums` once; a batch is one launch of `pcd_mesh_batch_clouds` (csrc/mesh_data.hip): `num_points`
    area-uniform surface points per mesh, new ones for every batch of every epoch, then the chain of `DeviceVoxelDataModule`
    (`augmentations` = jitter, `rotate` opt-in, `normalization` = centroid and unit radius last).  A batch is `(B, num_points, 3)`; with
    `return_normals` a pair (clouds, unit face normals, rotated with the points); with `return_labels` the int64 labels follow.  The
    category of a file is the subdirectory of `data_dir` that holds it ("" for files directly in it), `categories` the sorted distinct
    names, a label the index into them.  The split is `random_split` over the rows under the global torch generator; the per-epoch
    Philox key comes from that generator too, the validation loader's is fixed.
    `meshes=` (a list of `Mesh` / (vertices, faces) pairs) with optional integer `labels=` replaces `data_dir` (tests, synthetic runs);
    `device="cpu"` keeps the table on the host, where `setup()` works and the loaders do not."""

    def __init__(self, data_dir=None, num_points=2048, batch_size=32, train_val_split=0.8, augmentations=True, normalization=True,
                 rotate=False, return_labels=False, return_normals=False, device="cuda", meshes=None, labels=None,
                 jitter_sigma=0.01, jitter_clip=0.05):
        if (data_dir is None) == (meshes is None):
            raise ValueError("give either data_dir or meshes")
        if return_labels and meshes is not None and labels is None:
            raise ValueError("return_labels with meshes= needs labels=")
        if not 0 < int(num_points) <= MESH_MAX_POINTS:
            raise ValueError(f"num_points must be in 1..{MESH_MAX_POINTS}, got {num_points!r}")
        self.data_dir, self.num_points, self.batch_size, self.train_val_split = data_dir, int(num_points), batch_size, train_val_split
        self.augmentations, self.normalization, self.rotate = augmentations, normalization, bool(rotate)
        self.return_labels, self.return_normals = return_labels, return_normals
        self.device, self.meshes, self.labels = torch.device(device), meshes, labels
        self.jitter_sigma, self.jitter_clip = float(jitter_sigma), float(jitter_clip)
        self.flags = ((VOXEL_NORMALIZE if normalization else 0) | (VOXEL_JITTER if augmentations else 0)
                      | (VOXEL_ROTATE if rotate else 0))
        self.categories: List[str] = []

    @staticmethod
    def _checked(mesh, name: str):
        """(vertices float32 (V, 3), faces int32 (F, 3)) of one mesh on the host, or ValueError naming it."""
        v, f = mesh
        v = np.ascontiguousarray(torch.as_tensor(v).detach().cpu().numpy(), dtype=np.float32)
        f = np.ascontiguousarray(torch.as_tensor(f).detach().cpu().numpy())
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"{name}: not (V, 3) vertices and (F, 3) faces")
        if f.shape[0] == 0:
            raise ValueError(f"{name}: the mesh has no faces")
        if f.min() < 0 or f.max() >= v.shape[0]:
            raise ValueError(f"{name}: a face index is outside the mesh's {v.shape[0]} vertices")
        t = v.astype(np.float64)[f.astype(np.int64)]
        with np.errstate(all="ignore"):
            area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()
        if not np.isfinite(area) or not area > 0.0 or not area <= 3.0e38:
            raise ValueError(f"{name}: the total area of the mesh is {area}; a surface to draw from needs a positive finite area")
        return v, f.astype(np.int32)

    def setup(self, stage=None):
        if self.meshes is not None:
            names = [f"meshes[{i}]" for i in range(len(self.meshes))]
            raw = iter(self.meshes)
            labels = None if self.labels is None else [int(v) for v in self.labels]
            if labels is not None and len(labels) != len(names):
                raise ValueError(f"{len(labels)} labels for {len(names)} meshes")
        else:
            from .utils import load_mesh
            self.file_list = mesh_files(self.data_dir)
            names = [os.path.join(self.data_dir, f) for f in self.file_list]
            raw = (load_mesh(p) for p in names)
            self.categories = sorted({mesh_category(f) for f in self.file_list})
            labels = [self.categories.index(mesh_category(f)) for f in self.file_list] if self.return_labels else None
        if not names:
            raise ValueError(f"{self.data_dir}: no .obj or .ply file" if self.meshes is None else "meshes is empty")
        vs, fs, rows = [], [], [(0, 0)]
        for name, mesh in zip(names, raw):
            v, f = self._checked(mesh, name)
            vs.append(v)
            fs.append(f)
            rows.append((rows[-1][0] + v.shape[0], rows[-1][1] + f.shape[0]))
        self.offsets_host = np.asarray(rows, dtype=np.int64)
        self.vertices = torch.from_numpy(np.concatenate(vs)).to(self.device)
        self.faces = torch.from_numpy(np.concatenate(fs)).to(self.device)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.area_sums = None
        if self.device.type == "cuda":
            from . import _lib
            self.area_sums = torch.empty(self.faces.shape[0], dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().pcd_mesh_area_sums(_lib.ptr(self.vertices), _lib.ptr(self.faces), _lib.ptr(self.offsets), len(names),
                                                          _lib.ptr(self.area_sums), _lib.stream_ptr()), "mesh_area_sums")
        self.labels_device = None if labels is None else torch.as_tensor(labels, dtype=torch.int64, device=self.device)
        table = _Rows(len(names))
        train_size = int(self.train_val_split * len(table))
        self.train_dataset, self.val_dataset = torch.utils.data.random_split(table, [train_size, len(table) - train_size])

    def batch(self, index: torch.Tensor, seed: int, offset: int, return_faces: bool = False):
        """The batch of the table's rows `index` (device int32) under Philox key `seed`, slot b's counters starting at
        `offset + b * MESH_CTR_SPAN`: (B, num_points, 3) clouds; with `return_normals` (clouds, normals); `return_faces` (tests) appends
        the (B, num_points) int32 face of every point."""
        from . import _lib
        if self.area_sums is None:
            raise RuntimeError("DeviceMeshDataModule assembles batches on the GPU: construct it with device='cuda' (no CPU path)")
        lib, b, dev = _lib.load(), int(index.numel()), self.vertices.device
        out = torch.empty((b, self.num_points, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((b, self.num_points, 3), dtype=torch.float32, device=dev) if self.return_normals else None
        faces = torch.empty((b, self.num_points), dtype=torch.int32, device=dev) if return_faces else None
        _lib.check(lib.pcd_mesh_batch_clouds(_lib.ptr(self.vertices), _lib.ptr(self.faces), _lib.ptr(self.offsets), self.offsets.shape[0] - 1,
                                             _lib.ptr(self.area_sums), _lib.ptr(index), b, self.num_points, seed & 0xFFFFFFFFFFFFFFFF,
                                             offset & 0xFFFFFFFFFFFFFFFF, self.flags, self.jitter_sigma, self.jitter_clip, _lib.ptr(out),
                                             _lib.ptr(normals), _lib.ptr(faces), _lib.stream_ptr()), "mesh_batch_clouds")
        res = (out,) + ((normals,) if self.return_normals else ()) + ((faces,) if return_faces else ())
        return res[0] if len(res) == 1 else res

    def train_dataloader(self):
        return _DeviceLoader(self, self.train_dataset.indices, shuffle=True, ctr_span=MESH_CTR_SPAN)

    def val_dataloader(self):
        return _DeviceLoader(self, self.val_dataset.indices, shuffle=False, ctr_span=MESH_CTR_SPAN)
