"""`utils.load_mesh` on the host: what `save_mesh` writes comes back bit for bit, hand-written OBJ / PLY files load to the expected arrays, and every
refusal the loader documents raises ValueError (no GPU)."""
import struct

import numpy as np
import pytest
import torch

TETRA_V = np.asarray([[0.1, 0.2, 0.3], [1.0, 1e-7, -2.5], [1.0 / 3.0, 2.0 / 3.0, 123456.789], [-1.0, 0.0, 1.0]], np.float32)
TETRA_F = np.asarray([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)


@pytest.mark.parametrize("ext", ["obj", "ply"])
def test_save_then_load_returns_the_same_bits(tmp_path, ext):
    from shapegen_amd.utils import Mesh, load_mesh, save_mesh
    g = np.random.default_rng(0)
    cases = {"tetra": (TETRA_V, TETRA_F), "random": (g.standard_normal((50, 3)).astype(np.float32), g.integers(0, 50, (80, 3)).astype(np.int32)),
             "empty": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))}
    for name, (v, f) in cases.items():
        path = str(tmp_path / f"{name}.{ext}")
        save_mesh(path, (torch.from_numpy(v), torch.from_numpy(f)))
        m = load_mesh(path)
        assert isinstance(m, Mesh) and m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32
        assert m.vertices.device.type == "cpu" and tuple(m.vertices.shape) == v.shape and tuple(m.faces.shape) == f.shape, name
        assert np.array_equal(m.vertices.numpy().view(np.uint32), v.view(np.uint32)), name
        assert np.array_equal(m.faces.numpy(), f), name


def test_hand_written_obj(tmp_path):
    from shapegen_amd.utils import load_mesh
    path = tmp_path / "hand.OBJ"                                           # the extension is matched without case
    path.write_text("# a comment\nmtllib none.mtl\no thing\n"
                    "v 0 0 0\nv 1 0 0 1.0\nv 1 1 0\nv 0 1 0 0.5 0.5 0.5\n"
                    "vt 0 0\nvn 0 0 1\ns off\n"
                    "f 1/1/1 2/1/1 3/1/1\n"            # i/t/n
                    "f 1 2 3 4\n"                      # a quad
                    "v 0.5 2 0\n"
                    "f 1//1 2//1 3//1 5//1 4//1\n"     # a pentagon, i//n
                    "f -1 -2/1 -5\n"                   # negative: relative to the 5 vertices read so far
                    "usemtl x\ng y\n\n")
    m = load_mesh(str(path))
    assert np.array_equal(m.vertices.numpy(), np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 2, 0]], np.float32))
    assert m.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3], [4, 3, 0]]


def test_hand_written_ascii_ply_with_doubles_and_an_extra_property(tmp_path):
    from shapegen_amd.utils import load_mesh
    path = tmp_path / "hand.ply"
    path.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty double x\nproperty uchar red\nproperty double y\n"
                    "property double z\nelement face 2\nproperty list uchar int vertex_index\nend_header\n"
                    "0 255 0 0\n1 0 0 0.25\n1 7 1 0\n0 9 1 1e-3\n3 0 1 2\n4 0 1 2 3\n")
    m = load_mesh(str(path))
    assert np.array_equal(m.vertices.numpy(), np.asarray([[0, 0, 0], [1, 0, 0.25], [1, 1, 0], [0, 1, 1e-3]], np.float32))
    assert m.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3]]


def _binary_ply(count_fmt, count_name, item_fmt, item_name, extra_face_property=False, fmt="binary_little_endian"):
    header = (f"ply\nformat {fmt} 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty short flag\nproperty float z\n"
              f"element face 2\nproperty list {count_name} {item_name} vertex_indices\n" + ("property uchar flags\n" if extra_face_property else "")
              + "element edge 1\nproperty int a\nend_header\n")
    body = b"".join(struct.pack("<ffhf", x, y, 7, z) for x, y, z in ((0, 0, 0), (1, 0, 0), (1, 1, 0.5), (0, 1, 0)))
    body += struct.pack("<" + count_fmt + 3 * item_fmt, 3, 0, 1, 2) + (b"\x01" if extra_face_property else b"")
    body += struct.pack("<" + count_fmt + 4 * item_fmt, 4, 0, 2, 3, 1) + (b"\x01" if extra_face_property else b"")
    return header.encode("ascii") + body + struct.pack("<i", 5)          # the edge element that follows is left unread


@pytest.mark.parametrize("count,item", [(("H", "ushort"), ("i", "int")), (("B", "uchar"), ("H", "ushort")), (("i", "int"), ("I", "uint")),
                                        (("b", "char"), ("h", "short")), (("h", "short"), ("i", "int")), (("I", "uint"), ("i", "int"))])
def test_hand_written_binary_ply(tmp_path, count, item):
    from shapegen_amd.utils import load_mesh
    path = tmp_path / "hand.ply"
    path.write_bytes(_binary_ply(count[0], count[1], item[0], item[1]))
    m = load_mesh(str(path))
    assert np.array_equal(m.vertices.numpy(), np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]], np.float32))
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 1]]


def test_refusals_raise_value_error(tmp_path):
    from shapegen_amd.utils import load_mesh

    count = iter(range(100))

    def obj(text):
        p = tmp_path / f"bad{next(count)}.obj"
        p.write_text(text)
        return str(p)

    def ply(data):
        p = tmp_path / f"bad{next(count)}.ply"
        p.write_bytes(data if isinstance(data, bytes) else data.encode("ascii"))
        return str(p)

    square = "v 0 0 0\nv 1 0 0\nv 1 1 0\n"
    ascii_head = "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
    rows = "0 0 0\n1 0 0\n1 1 0\n"
    cases = [(obj(square + "f 1 2 4\n"), "out of range"),                      # beyond the vertices read so far
             (obj(square + "f 1 2 0\n"), "out of range"),                      # 0 is no index
             (obj(square + "f -4 1 2\n"), "out of range"),                     # further back than the first vertex
             (obj(square + "f 1 2\n"), "fewer than 3"),
             (obj("f 1 2 3\n" + square), "out of range"),                      # faces see only the vertices read so far
             (ply(ascii_head + "property list uchar int vertex_indices\nend_header\n" + rows + "3 0 1 3\n"), "out of range"),
             (ply(ascii_head + "property list uchar int vertex_indices\nend_header\n" + rows + "2 0 1\n"), "fewer than 3"),
             (ply(_binary_ply("B", "uchar", "i", "int", fmt="binary_big_endian")), "big_endian"),
             (ply(_binary_ply("B", "uchar", "i", "int", extra_face_property=True)), "additional face properties"),
             (str(tmp_path / "mesh.stl"), "reads .obj or .ply")]
    for path, why in cases:
        with pytest.raises(ValueError, match=why) as e:
            load_mesh(path)
        assert path in str(e.value)                                         # the message names the file
