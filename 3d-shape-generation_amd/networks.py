"""Denoiser / VAE modules with the reference's constructor signatures and `state_dict`
contract (reference networks.py), executing on hand-written gfx950 kernels.

The modules are parameter containers (a `ParamTree` generated from `specs`) plus a
packed device-side weight cache; `forward` enqueues HIP kernels through the C ABI
(`_lib`).  There is no PyTorch compute path and no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, packing, specs


# --------------------------------------------------------------------------- params
class _Node(nn.Module):
    pass


class ParamTree(nn.Module):
    """nn.Module whose parameters/buffers are generated from a spec list so that
    `state_dict()` has exactly the reference's keys, shapes and order."""

    def _build_from_spec(self, spec: specs.Spec) -> None:
        for key, shape, role in spec:
            parts = key.split(".")
            node: nn.Module = self
            for name in parts[:-1]:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            leaf = parts[-1]
            if role in ("w", "wT"):
                t = torch.empty(shape)
                # kaiming-normal fan_out (reference diffusion.py:44-48); fan_out = shape[0] * receptive field
                fan_out = shape[0] * int(np.prod(shape[2:]))   # torch's definition, transposed convs included
                t.normal_(0.0, math.sqrt(2.0 / max(fan_out, 1)))
                node.register_parameter(leaf, nn.Parameter(t))
            elif role in ("b", "beta"):
                node.register_parameter(leaf, nn.Parameter(torch.zeros(shape)))
            elif role == "g":
                node.register_parameter(leaf, nn.Parameter(torch.ones(shape)))
            elif role == "rm":
                node.register_buffer(leaf, torch.zeros(shape))
            elif role == "rv":
                node.register_buffer(leaf, torch.ones(shape))
            elif role == "nbt":
                node.register_buffer(leaf, torch.tensor(0, dtype=torch.long))
            else:
                raise ValueError(role)


class _HipModule(ParamTree):
    """Common machinery: packed-weight cache invalidation, the C handles made from the packed weights, and device checks."""

    def __init__(self):
        super().__init__()
        self._packed = None
        self._handle = None                 # the module's C handle, while packed
        self._owned = []                    # (destroy, handle) of every C handle made from the packed weights, in creation order
        self._ws: Dict[tuple, torch.Tensor] = {}
        # a parent's load_state_dict recurses through _load_from_state_dict and never calls a child's
        # load_state_dict override: the post hook fires for every module that received keys
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate())

    def invalidate(self) -> None:
        """Drop the packed device weights (call after mutating parameters in place)."""
        self._release()
        self._packed = None
        self._ws = {}

    def _create(self, create, destroy, desc) -> C.c_void_p:
        """The handle `create(&desc, &handle)` makes; `invalidate` and garbage collection pass it to `destroy`."""
        handle = C.c_void_p()
        _lib.check(create(C.byref(desc), C.byref(handle)), create.__name__)
        self._owned.append((destroy, handle))
        return handle

    def _release(self) -> None:
        owned, self._owned, self._handle = self._owned, [], None
        for destroy, handle in owned:
            destroy(handle)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self.invalidate()
        return super().load_state_dict(*a, **k)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def _need_cuda(self, *tensors) -> torch.device:
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs only on an MI355X device; call .to('cuda') "
                               "(this framework has no CPU path)")
        for t in tensors:
            if t is not None and t.device != dev:
                raise RuntimeError(f"input on {t.device}, module on {dev}")
        return dev

    def _workspace(self, key: tuple, nbytes: int) -> torch.Tensor:
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws = {key: ws}   # keep only the latest shape's workspace
        return ws


def _dev16(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16).to(dev).contiguous()


def _dev32(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dev).contiguous()


class _Denoiser(_HipModule):
    """`precision`: "fp16" (default; fp16 operands on the matrix cores, fp32 accumulation) or "fp32" (SURVEY 8(c)'s parity
    mode: fp32 weights, activations and products -- the reference's own arithmetic type, held to eps rel-L2 <= 1e-4).  Chosen
    per module with `set_precision`, or for every module created afterwards with the environment variable PCD_PARITY=fp32."""

    PRECISIONS = ("fp16", "fp32")

    def __init__(self):
        super().__init__()
        self.precision = os.environ.get("PCD_PARITY", "fp16")
        if self.precision not in self.PRECISIONS:
            raise ValueError(f"PCD_PARITY must be one of {self.PRECISIONS}, got {self.precision!r}")

    def set_precision(self, precision: str):
        """Switch to "fp16" or "fp32"; a change drops the packed weights."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {self.PRECISIONS}, got {precision!r}")
        if precision != self.precision:
            self.invalidate()
            self.precision = precision
        return self

    @property
    def _dtype(self) -> torch.dtype:
        """The activation type of the active precision."""
        return torch.float32 if self.precision == "fp32" else torch.float16


class _HandleDenoiser(_Denoiser):
    """A denoiser behind a C handle: eps = forward_with_bias(x, time_bias(t), 1), one C call once the time bias is known.
    `_ensure_packed` creates the handle of the active precision and binds the entry points that run on it (`_bind`)."""

    def _bind(self, desc, create, destroy, workspace_bytes, forward, tap=None) -> C.c_void_p:
        """Make the handle of `desc`; `forward_with_bias` and `_tap` call `forward` / `tap` on it from now on."""
        handle = self._create(create, destroy, desc)
        self._entry = (handle, workspace_bytes, forward, tap)
        return handle

    def forward_with_bias(self, x: torch.Tensor, tbias: torch.Tensor, shape_stride: int,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eps for x (B,N,3) -- z (B,latent) for the latent denoiser -- given a precomputed time bias row (stride 0) or one
        row per shape (1)."""
        self._ensure_packed()
        handle, workspace_bytes, forward, _ = self._entry
        dims = x.shape[:-1]
        if out is None:
            out = torch.empty_like(x)
        ws = self._workspace(dims, workspace_bytes(*dims))
        _lib.check(forward(handle, x.data_ptr(), *dims, tbias.data_ptr(), shape_stride, out.data_ptr(), ws.data_ptr(), ws.numel(),
                           _lib.stream_ptr()), forward.__name__)
        return out

    def check_labels(self, labels, batch: int) -> Optional[torch.Tensor]:
        """Host-side validation of a label argument: None on a model without classes, else (batch,) int32 on the device with
        values in [0, num_classes] (`None` = the null class `num_classes` for every shape)."""
        if not getattr(self, "num_classes", 0):
            if labels is not None:
                raise ValueError("labels were given to a model without classes (num_classes=0)")
            return None
        if labels is None:
            return torch.full((batch,), self.num_classes, dtype=torch.int32, device=self.device)
        lab = torch.as_tensor(labels)
        if lab.is_floating_point() or lab.is_complex() or lab.dtype == torch.bool:
            raise ValueError(f"labels must be integers, got {lab.dtype}")
        if lab.dim() != 1 or lab.shape[0] != batch:
            raise ValueError(f"labels must be ({batch},), got {tuple(lab.shape)}")
        if batch and (int(lab.min()) < 0 or int(lab.max()) > self.num_classes):
            raise ValueError(f"labels must lie in [0, {self.num_classes}] ({self.num_classes} = unconditional), got "
                             f"[{int(lab.min())}, {int(lab.max())}]")
        return lab.to(self.device, torch.int32).contiguous()

    def _tap(self, name: str, batch: int, n_points: int, ws: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        handle, _, _, tap = self._entry
        _lib.check(tap(handle, name.encode(), batch, n_points, ws.data_ptr(), dst.data_ptr(), dst.numel() * dst.element_size(),
                       _lib.stream_ptr()), tap.__name__)
        return dst


def _time_embed(m: _HandleDenoiser, t: torch.Tensor, mlp_dim: int, c1: int = 0) -> torch.Tensor:
    """pcd_time_embed on m's packed time MLP: time_mlp(get_timestep_embedding(t)) as (len(t), mlp_dim) fp32, or with c1 > 0
    the hoisted time half of enc1 as (len(t), c1) fp32."""
    pk = m._ensure_packed()
    t = t.to(m.device, torch.float32).contiguous()
    out = torch.empty(t.numel(), c1 or mlp_dim, dtype=torch.float32, device=m.device)
    if c1:
        temb, e1w_t, e1b, tbias = 0, pk["e1w_t"].data_ptr(), pk["e1b"].data_ptr(), out.data_ptr()
    else:
        temb, e1w_t, e1b, tbias = out.data_ptr(), 0, 0, 0
    _lib.check(_lib.load().pcd_time_embed(
        t.data_ptr(), t.numel(), pk["freqs"].data_ptr(), m.time_dim, mlp_dim,
        pk["tw0"].data_ptr(), pk["tb0"].data_ptr(), pk["tw2"].data_ptr(), pk["tb2"].data_ptr(),
        temb, e1w_t, e1b, c1, tbias, _lib.stream_ptr()), "time_embed")
    return out


# ------------------------------------------------------------------ UNetPointNetLarge
class UNetPointNetLarge(_HandleDenoiser):
    """Drop-in for reference networks.py:724-838: eps = model(x (B,N,3), t (B,)).  fp16 mode: csrc/unet.hip, fp32 mode:
    csrc/unet_f32.hip (see `_Denoiser`).  The constructor signature stays the reference's but for `num_classes` (not in the
    reference): with num_classes > 0 the module owns `class_emb`, an nn.Embedding(num_classes + 1, dim) registered after the
    reference's modules (row `num_classes` is the null class of classifier-free guidance), and
    temb_b = time_mlp(sinusoid(t_b)) + class_emb[label_b].  time enters only as the per-shape bias of enc1.conv1 and that product
    is linear, so the class term is one more hoisted bias (`class_bias`)."""

    def __init__(self, dim: int = 512, time_dim: int = 256, num_classes: int = 0):
        super().__init__()
        self.dim, self.time_dim = dim, time_dim
        self.num_classes = int(num_classes)
        if self.num_classes < 0:
            raise ValueError(f"num_classes must be >= 0, got {num_classes}")
        self._build_from_spec(specs.unet_pointnet_large_spec(dim, time_dim))
        if self.num_classes:
            self.class_emb = nn.Embedding(self.num_classes + 1, dim)
        # fp16 mode: the narrow layers at the two ends of the U-net (enc1.conv2/3, enc2.conv3, dec1.*, output.0: the direct route from
        # the coordinates to the predicted noise) carry hi / lo weights -- the fp16 weights and the fp16 of their rounding residuals,
        # two MFMA passes, < 2 % of the FLOPs -- because the fp16 rounding of THESE weights is what the 1000-step DDPM trajectory
        # deviated by.  PCD_NARROW_HILO=0 / set_hilo_mask(0): plain fp16 weights everywhere.
        self.hilo_mask = _lib.PCD_UNET_HILO_ALLOWED if os.environ.get("PCD_NARROW_HILO", "1") != "0" else 0

    def set_hilo_mask(self, mask: int) -> "UNetPointNetLarge":
        if mask & ~_lib.PCD_UNET_HILO_ALLOWED:
            raise ValueError(f"hi / lo weights are available for layers {_lib.PCD_UNET_HILO_ALLOWED:#x} only, got {mask:#x}")
        if mask != self.hilo_mask:
            self.invalidate()
            self.hilo_mask = mask
        return self

    # -- packing -----------------------------------------------------------------
    def _ensure_packed(self):
        if self._packed is not None:
            return self._packed
        dev = self._need_cuda()
        _lib.require_gpu()
        lib = _lib.load()
        f32 = self.precision == "fp32"
        devw = _dev32 if f32 else _dev16
        lin, ex = packing.pack_point_unet(self.state_dict(), "", self.time_dim, self.dim)
        keep = {"freqs": packing.timestep_freqs(self.time_dim).to(dev)}
        for k in ("tw0", "tb0", "tw2", "tb2", "e1w_xyz", "e1w_t", "e1b", "head_w", "head_b"):
            keep[k] = _dev32(ex[k], dev)
        keep["wg"] = devw(ex["wg"], dev)
        desc = _lib.UnetDesc()
        desc.time_dim, desc.dim = self.time_dim, self.dim
        for k in ("freqs", "tw0", "tb0", "tw2", "tb2", "e1w_xyz", "e1w_t", "e1b", "head_w", "head_b", "wg"):
            setattr(desc, k, keep[k].data_ptr())
        desc.wg_k, desc.wg_c = 4096, 1024
        desc.hilo_mask = 0 if f32 else self.hilo_mask
        for i, (w, b) in enumerate(lin):
            if (desc.hilo_mask >> i) & 1:
                keep[f"w{i}"] = _dev16(packing.split_hilo(w), dev)                   # [C][2 K] = hi | lo
            else:
                keep[f"w{i}"] = devw(w, dev)
            keep[f"b{i}"] = _dev32(b, dev)
            desc.lin[i].w, desc.lin[i].b = keep[f"w{i}"].data_ptr(), keep[f"b{i}"].data_ptr()
            desc.lin[i].c, desc.lin[i].k = w.shape
        if f32:
            self._handle = self._bind(desc, lib.pcd_unet_f32_create, lib.pcd_unet_f32_destroy, lib.pcd_unet_f32_workspace_bytes,
                                      lib.pcd_unet_f32_forward, lib.pcd_unet_f32_tap)
        else:
            self._handle = self._bind(desc, lib.pcd_unet_create, lib.pcd_unet_destroy, lib.pcd_unet_workspace_bytes,
                                      lib.pcd_unet_forward, lib.pcd_unet_tap)
        self._packed = keep
        return keep

    # -- pieces used by the samplers ---------------------------------------------------
    def time_bias(self, t: torch.Tensor) -> torch.Tensor:
        """Hoisted time half of enc1.conv1 for each value of t: (len(t), 64) fp32 (K3)."""
        return _time_embed(self, t, self.dim, 64)

    def time_mlp_out(self, t: torch.Tensor) -> torch.Tensor:
        """time_mlp(get_timestep_embedding(t)) (networks.py:791-792), for parity tests."""
        return _time_embed(self, t, self.dim)

    def class_bias(self) -> torch.Tensor:
        """Hoisted class half of enc1.conv1: the folded time columns applied to every row of `class_emb`, without the bias
        term (`time_bias` carries it), (num_classes + 1, 64) fp32.  It goes through the packed weights `time_bias` uses and
        is kept with them, so it is rebuilt whenever they are."""
        if not self.num_classes:
            raise RuntimeError("class_bias needs a class-conditional model (num_classes > 0)")
        pk = self._ensure_packed()
        if "class_bias" not in pk:
            emb = self.class_emb.weight.detach().to(torch.float32).contiguous()
            out = torch.empty(emb.shape[0], 64, dtype=torch.float32, device=self.device)
            _lib.check(_lib.load().pcd_linear_f32(emb.data_ptr(), emb.shape[0], self.dim, pk["e1w_t"].data_ptr(), None, 64, out.data_ptr(),
                                                  _lib.stream_ptr()), "linear_f32")
            pk["class_bias"] = out
        return pk["class_bias"]

    def forward(self, x: torch.Tensor, t: torch.Tensor, labels=None) -> torch.Tensor:
        self._need_cuda(x, t)
        if x.dim() != 3 or x.shape[2] != 3:
            raise ValueError(f"x must be (B, N, 3), got {tuple(x.shape)}")
        if t.dim() != 1 or t.shape[0] != x.shape[0]:
            raise ValueError(f"t must be (B,), got {tuple(t.shape)} for batch {x.shape[0]}")
        x = x.to(torch.float32).contiguous()
        tb = self.time_bias(t)
        if getattr(self, "num_classes", 0) or labels is not None:
            if not hasattr(self, "check_labels"):
                raise ValueError("labels were given to a model without classes")
            lab = self.check_labels(labels, x.shape[0])
            cb = self.class_bias()
            _lib.check(_lib.load().pcd_embed_add_rows(tb.data_ptr(), cb.data_ptr(), lab.data_ptr(), x.shape[0], 64, cb.shape[0],
                                                      _lib.stream_ptr()), "embed_add_rows")
        return self.forward_with_bias(x, tb, 1)

    _TAP_WIDTHS = {"x1": 128, "x2": 256, "x3": 512, "x4": 1024, "d4": 512, "d3": 256, "d2": 128, "d1": 64}

    def capture_decoder(self, batch: int, n_points: int, on: bool = True) -> None:
        """fp16 path, parity tests: make the following forwards of this shape keep the decoder blocks' outputs
        (dec4..dec1, networks.py:811-814) for `tap("d4".."d1")`; they otherwise live in ping-pong buffers and inside
        the chained tail.  The fp32 path always keeps them."""
        pk = self._ensure_packed()
        if self.precision == "fp32":
            return
        if on:
            pk["capture"] = {k: torch.empty(batch, n_points, self._TAP_WIDTHS[k], dtype=torch.float16, device=self.device)
                             for k in ("d4", "d3", "d2", "d1")}
            ptrs = [pk["capture"][k].data_ptr() for k in ("d4", "d3", "d2", "d1")]
        else:
            pk["capture"], ptrs = None, [0, 0, 0, 0]
        _lib.check(_lib.load().pcd_unet_capture(self._handle, *ptrs), "unet_capture")

    def tap(self, name: str, batch: int, n_points: int) -> torch.Tensor:
        """Intermediate of the last forward (parity tests): x1..x4 / d4..d1 as (B,N,C) (fp16, or fp32 in the fp32 mode),
        pooled / gbias fp32."""
        ws = self._ws[(batch, n_points)]
        if name in self._TAP_WIDTHS:
            if self.precision == "fp16" and name.startswith("d"):     # the fp16 library keeps them only in capture_decoder's buffers
                capture = self._packed.get("capture")
                if capture is None or tuple(capture[name].shape[:2]) != (batch, n_points):
                    raise RuntimeError("decoder taps of the fp16 path need capture_decoder(batch, n_points) before the forward")
                return capture[name].clone()
            dst = torch.empty(batch, n_points, self._TAP_WIDTHS[name], dtype=self._dtype, device=self.device)
        else:
            dst = torch.empty(batch, {"pooled": 4096, "gbias": 1024}[name], dtype=torch.float32, device=self.device)
        return self._tap(name, batch, n_points, ws, dst)


# ------------------------------------------------------------------ set attention
class _PackedSAB:
    """Device weights of one SetAttentionBlock (reference networks.py:51-68) and their C descriptor."""

    def __init__(self, sd, prefix: str, dim: int, dev, f32: bool = False):
        g = lambda k: sd[prefix + k].detach().to("cpu", torch.float64).numpy()
        devw = _dev32 if f32 else _dev16                                   # fp32 parity mode: fp32 weights (csrc/attn_f32.hip)
        self.dim = dim
        self.w_in, self.b_in = devw(g("attention.in_proj_weight"), dev), _dev32(g("attention.in_proj_bias"), dev)
        self.w_out, self.b_out = devw(g("attention.out_proj.weight"), dev), _dev32(g("attention.out_proj.bias"), dev)
        self.ln1_g, self.ln1_b = _dev32(g("ln1.weight"), dev), _dev32(g("ln1.bias"), dev)
        self.ln2_g, self.ln2_b = _dev32(g("ln2.weight"), dev), _dev32(g("ln2.bias"), dev)
        self.w_ff1, self.b_ff1 = devw(g("ff.0.weight"), dev), _dev32(g("ff.0.bias"), dev)
        self.w_ff2, self.b_ff2 = devw(g("ff.2.weight"), dev), _dev32(g("ff.2.bias"), dev)
        self.packed = {}                                                   # descriptor field -> the packed buffer it points to
        self.f32 = f32

    def fill(self, d: "_lib.SabDesc") -> "_lib.SabDesc":
        d.dim = self.dim
        for k in ("w_in", "b_in", "w_out", "b_out", "ln1_g", "ln1_b", "ln2_g", "ln2_b", "w_ff1", "b_ff1", "w_ff2", "b_ff2"):
            setattr(d, k, getattr(self, k).data_ptr())
        lib = _lib.load()
        p = lambda *names: [getattr(self, n).data_ptr() for n in names]
        # fp16 only: (descriptor field, bytes, packer(destination, stream)) of the fragment-order stage images a fused launch reads
        fused = []
        if not self.f32:
            # C <= 128 (0 bytes otherwise): the block's head (LN1 + in_proj) and tail (out_proj + residual + LN2 + FFN + residual) as one launch each
            fused.append(("tail_packed", lib.pcd_sab_tail_packed_bytes(self.dim), lambda dst, st: lib.pcd_sab_tail_pack(C.byref(d), dst, st)))
        if self.dim == 256 and not self.f32:
            # LN1 + in_proj and LN2 + ff.0 as one launch each (wide-chain kernel with a LayerNorm prologue) ...
            ln_linear = lambda passes, *names: (lib.pcd_pw_wide_ln_linear_packed_bytes(passes),
                                                lambda dst, st: lib.pcd_pw_wide_ln_linear_pack(*p(*names[:2]), passes, *p(*names[2:]), dst, st))
            fused.append(("ln_in_packed", *ln_linear(3, "w_in", "b_in", "ln1_g", "ln1_b")))
            fused.append(("ln_ff1_packed", *ln_linear(4, "w_ff1", "b_ff1", "ln2_g", "ln2_b")))
            # ... and LN2 + ff.0 + ReLU + ff.2 + residual as ONE launch (csrc/wideffn.hip): the 4C-wide hidden tensor is never written
            fused.append(("ffn_packed", lib.pcd_wide_ffn_packed_bytes(),
                          lambda dst, st: lib.pcd_wide_ffn_pack(*p("w_ff1", "b_ff1", "w_ff2", "b_ff2", "ln2_g", "ln2_b"), dst, st)))
        packed_now = False
        for field in ("tail_packed", "ln_in_packed", "ln_ff1_packed", "ffn_packed"):
            setattr(d, field, None)
        for field, nbytes, pack in fused:
            if not nbytes:
                continue
            if field not in self.packed:
                buf = torch.empty(nbytes, dtype=torch.uint8, device=self.w_out.device)
                _lib.check(pack(buf.data_ptr(), _lib.stream_ptr()), field)
                self.packed[field] = buf
                packed_now = True
            setattr(d, field, self.packed[field].data_ptr())
        if packed_now:
            # the images were written by pack kernels on the CURRENT stream; a forward enqueued on another stream (a side stream, a capture) must find them
            # complete: one synchronisation per model packing
            torch.cuda.current_stream().synchronize()
        return d


class SetAttentionBlock(_Denoiser):
    """Drop-in for reference networks.py:51-83: (B, N, C) -> (B, N, C), pre-LN MHA + FFN, one pcd_sab_forward call
    (fp16: flash-style kernel on the matrix cores; fp32: csrc/attn_f32.hip)."""

    def __init__(self, dim: int, num_heads: int):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self._build_from_spec(specs.set_attention_spec(dim))

    def _ensure_packed(self):
        if self._packed is None:
            dev = self._need_cuda()
            _lib.require_gpu()
            lib = _lib.load()
            f32 = self.precision == "fp32"
            pk = _PackedSAB(self.state_dict(), "", self.dim, dev, f32=f32)
            entry = (lib.pcd_sab_f32_workspace_bytes, lib.pcd_sab_f32_forward) if f32 else (lib.pcd_sab_workspace_bytes, lib.pcd_sab_forward)
            self._packed = (pk, pk.fill(_lib.SabDesc()), *entry)
        return self._packed

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._need_cuda(x)
        b, n, c = x.shape
        if c != self.dim:
            raise ValueError(f"expected {self.dim} channels, got {c}")
        _, desc, workspace_bytes, forward = self._ensure_packed()
        xa = x.to(self._dtype).contiguous().reshape(b * n, c)
        y = torch.empty_like(xa)
        ws = self._workspace((b, n), workspace_bytes(b * n, c))
        _lib.check(forward(C.byref(desc), xa.data_ptr(), b, n, self.num_heads, y.data_ptr(), ws.data_ptr(), ws.numel(),
                           _lib.stream_ptr()), forward.__name__)
        return y.reshape(b, n, c).to(x.dtype)


class UNetAttentionPointExperimental(_HandleDenoiser):
    """Drop-in for reference networks.py:597-722 (the carrier of the set-attention blocks): eps = model(x (B,N,3), t (B,)).
    One pcd_attn_unet_forward call per forward; `time_bias` / `forward_with_bias` give the samplers the same two-stage
    surface as UNetPointNetLarge (the whole time path once per sampler call, one 704-float row per timestep).  fp32 mode:
    fp32 weights / activations / arithmetic, csrc/attn_f32.hip."""

    TB = _lib.PCD_ATTN_UNET_TB

    def __init__(self, num_points, dim=256, num_heads=4, num_blocks=3, time_dim=256):
        super().__init__()
        self.num_points, self.dim, self.num_heads, self.time_dim = num_points, dim, num_heads, time_dim
        self._build_from_spec(specs.unet_attention_spec(dim, time_dim))

    def _ensure_packed(self):
        if self._packed is not None:
            return self._packed
        if self.dim != self.time_dim:
            raise RuntimeError("UNetAttentionPointExperimental needs dim == time_dim: emb* layers take time_dim "
                               "inputs but receive time_mlp's dim outputs (reference networks.py:613-624,664-668)")
        dev = self._need_cuda()
        _lib.require_gpu()
        sd = self.state_dict()
        g = lambda k: sd[k].detach().to("cpu", torch.float64).numpy()
        keep = {"freqs": packing.timestep_freqs(self.time_dim).to(dev)}
        desc = _lib.AttnUnetDesc()
        desc.dim, desc.time_dim, desc.heads = self.dim, self.time_dim, self.num_heads
        desc.freqs = keep["freqs"].data_ptr()
        for name, field in (("time_mlp.0", "t*0"), ("time_mlp.2", "t*2")):
            keep[name + ".w"], keep[name + ".b"] = _dev32(g(name + ".weight"), dev), _dev32(g(name + ".bias"), dev)
            setattr(desc, field.replace("*", "w"), keep[name + ".w"].data_ptr())
            setattr(desc, field.replace("*", "b"), keep[name + ".b"].data_ptr())
        for i, (name, _) in enumerate(specs.ATTN_UNET_EMB):
            keep[name + ".w"], keep[name + ".b"] = _dev32(g(name + ".weight"), dev), _dev32(g(name + ".bias"), dev)
            desc.emb_w[i], desc.emb_b[i] = keep[name + ".w"].data_ptr(), keep[name + ".b"].data_ptr()
        # enc1 = PointNetLayer(3, 64): the K=3 first conv runs in the xyz kernel
        w, b = packing.fold_conv_bn(sd, "enc1.conv1", "enc1.bn1")
        keep["e1w"], keep["e1b"] = _dev32(w, dev), _dev32(b, dev)
        desc.e1w, desc.e1b = keep["e1w"].data_ptr(), keep["e1b"].data_ptr()
        stages = [("enc1", 2), ("enc1", 3)] + [(n, i) for n in ("enc2", "enc3", "dec3", "dec2") for i in (1, 2, 3)]
        for j, (name, i) in enumerate(stages):
            w, b = packing.fold_conv_bn(sd, f"{name}.conv{i}", f"{name}.bn{i}")
            keep[f"w{j}"], keep[f"b{j}"] = _dev16(w, dev), _dev32(b, dev)
            desc.lin[j].w, desc.lin[j].b = keep[f"w{j}"].data_ptr(), keep[f"b{j}"].data_ptr()
            desc.lin[j].c, desc.lin[j].k = w.shape
        for j, (name, c) in enumerate((("att1", 64), ("att2", 128), ("att3", 256), ("bottleneck", 256), ("att_dec3", 256),
                                       ("att_dec2", 128), ("att_dec1", 64))):
            keep[name] = _PackedSAB(sd, name + ".", c, dev)
            keep[name].fill(desc.sab[j])
        # tail: dec1 = PointNetLayer(128, 3, 3) + output Conv1d(3,3)
        w1, b1 = packing.fold_conv_bn(sd, "dec1.conv1", "dec1.bn1")
        w2, b2 = packing.fold_conv_bn(sd, "dec1.conv2", "dec1.bn2")
        w3, b3 = packing.fold_conv_bn(sd, "dec1.conv3", "dec1.bn3")
        w4, b4 = packing.fold_conv_bn(sd, "output", None)
        keep["t_w1"], keep["t_b1"] = _dev32(w1, dev), _dev32(b1, dev)
        keep["t_w234"] = _dev32(np.stack([w2, w3, w4]), dev)
        keep["t_b234"] = _dev32(np.stack([b2, b3, b4]), dev)
        for k in ("t_w1", "t_b1", "t_w234", "t_b234"):
            setattr(desc, k, keep[k].data_ptr())
        lib = _lib.load()
        # the time path is fp32 in both modes and runs on this handle (pcd_attn_unet_time_bias)
        self._handle = self._bind(desc, lib.pcd_attn_unet_create, lib.pcd_attn_unet_destroy, lib.pcd_attn_unet_workspace_bytes,
                                  lib.pcd_attn_unet_forward, lib.pcd_attn_unet_tap)
        if self.precision == "fp32":
            # the fp32 parity mode: a second descriptor whose layer / attention weights are fp32
            d32 = _lib.AttnUnetDesc()
            C.memmove(C.byref(d32), C.byref(desc), C.sizeof(desc))
            for j, (name, i) in enumerate(stages):
                w, b = packing.fold_conv_bn(sd, f"{name}.conv{i}", f"{name}.bn{i}")
                keep[f"w32_{j}"] = _dev32(w, dev)
                d32.lin[j].w = keep[f"w32_{j}"].data_ptr()
            for j, (name, c) in enumerate((("att1", 64), ("att2", 128), ("att3", 256), ("bottleneck", 256), ("att_dec3", 256),
                                           ("att_dec2", 128), ("att_dec1", 64))):
                keep[name + "_32"] = _PackedSAB(sd, name + ".", c, dev, f32=True)
                keep[name + "_32"].fill(d32.sab[j])
            self._bind(d32, lib.pcd_attn_unet_f32_create, lib.pcd_attn_unet_f32_destroy, lib.pcd_attn_unet_f32_workspace_bytes,
                       lib.pcd_attn_unet_f32_forward, lib.pcd_attn_unet_f32_tap)
        self._packed = keep
        return keep

    def time_bias(self, t: torch.Tensor) -> torch.Tensor:
        """Every time-dependent vector of the network for each value of t: (len(t), 704) fp32 rows
        [enc1 bias | emb2 | emb3 | emb_dec3 | emb_dec2 | emb_dec1] (networks.py:664-698)."""
        self._ensure_packed()
        t = t.to(self.device, torch.float32).contiguous()
        out = torch.empty(t.numel(), self.TB, dtype=torch.float32, device=self.device)
        scratch = torch.empty(t.numel(), self.dim, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().pcd_attn_unet_time_bias(self._handle, t.data_ptr(), t.numel(), scratch.data_ptr(),
                                                       out.data_ptr(), _lib.stream_ptr()), "attn_unet_time_bias")
        return out

    forward = UNetPointNetLarge.forward

    def tap(self, name: str, batch: int, n_points: int) -> torch.Tensor:
        """Skip tensor of the last forward (parity tests): x1 / x2 / x3 as (B, N, 64 / 128 / 256) fp16 (fp32 in the fp32 parity mode)."""
        ws = self._ws[(batch, n_points)]
        dst = torch.empty(batch, n_points, {"x1": 64, "x2": 128, "x3": 256}[name], dtype=self._dtype, device=self.device)
        return self._tap(name, batch, n_points, ws, dst)


# ------------------------------------------------------------------ latent denoiser
class SimpleLatentUNetPointNet(_HandleDenoiser):
    """Drop-in for reference networks.py:962-1106: eps = model(z (B, latent), t (B,)).
    Eval-mode only (Dropout(0.1) in dec1 is the identity, as in every sampler).  fp16 mode: the per-layer launches or the
    persistent kernel; fp32 mode: one launch per layer, csrc/latent_f32.hip (see `_Denoiser`).  `num_classes` (not in the
    reference) > 0: the module owns `class_emb`, an nn.Embedding(num_classes + 1, time_dim) registered after the reference's
    modules (row `num_classes` is the null class), and te_b = time_mlp(sinusoid(t_b)) + class_emb[label_b].  Time enters only
    through enc1's time columns and that product is linear, so the class term is one more hoisted bias (`class_bias`)."""

    def __init__(self, latent_dim, dim=512, time_dim=256, dropout_rate=0.1, num_classes=0):
        super().__init__()
        self.latent_dim, self.dim, self.time_dim = latent_dim, dim, time_dim
        self.num_classes = int(num_classes)
        if self.num_classes < 0:
            raise ValueError(f"num_classes must be >= 0, got {num_classes}")
        self._build_from_spec(specs.latent_unet_spec(latent_dim, dim, time_dim))
        if self.num_classes:
            self.class_emb = nn.Embedding(self.num_classes + 1, time_dim)

    # ------------------------------------------------------------------ the whole step as one persistent launch
    def persist_supported(self, batch: int) -> bool:
        """True when `csrc/latent_persist.hip` can run on this device for this batch (batch <= 64, a 256-CU gfx950)."""
        self._need_cuda()
        if self.precision != "fp16":
            return False                                   # the persistent kernel is an fp16-operand kernel
        return bool(_lib.load().pcd_latent_persist_supported(int(batch)))

    def _persist_handle(self):
        pk = self._ensure_packed()
        if "persist" not in pk:
            lib = _lib.load()
            pk["persist"] = self._create(lib.pcd_latent_persist_create, lib.pcd_latent_persist_destroy, pk["desc"])
            # its own buffer: the per-layer path keeps `_ws`
            pk["persist_ws"] = torch.empty(lib.pcd_latent_persist_workspace_bytes(pk["persist"]), dtype=torch.uint8, device=self.device)
        return pk["persist"], pk["persist_ws"]

    def persist_status(self) -> int:
        """Waits for the current stream (the one the launch was enqueued on) and returns the status word of the last persistent launch: 0 = every wait was met, else
        (wait kind << 16) | workgroup -- the launch was abandoned (0.2 s bound per wait) and its outputs are undefined."""
        h, ws = self._persist_handle()
        st = C.c_uint(0)
        _lib.check(_lib.load().pcd_latent_persist_status(ws.data_ptr(), C.byref(st), _lib.stream_ptr()), "latent_persist_status")
        return int(st.value)

    def check_persist_status(self):
        """Raises if the last persistent launch was abandoned (callers with no saved input to re-run from)."""
        st = self.persist_status()
        if st:
            raise RuntimeError(f"persistent latent kernel: wait kind {st >> 16} of workgroup {st & 0xffff} timed out "
                               "(is another process holding CUs of this GPU?  set PCD_LATENT_PERSISTENT=0 to use the per-layer launches)")

    def inject_persist_fault(self, workgroup: int, step: int = 0) -> None:
        """Recovery tests: workgroup `workgroup` of the following persistent launches leaves at step `step` (-1: off)."""
        h, _ = self._persist_handle()
        _lib.check(_lib.load().pcd_latent_persist_inject_fault(h, int(workgroup), int(step)), "latent_persist_inject_fault")

    def forward_persist(self, z, tbias_row, out=None):
        """eps = model(z, t) for ONE t shared by the batch (tbias_row = time_bias(t)[0], 128 values), one launch."""
        h, ws = self._persist_handle()
        if out is None:
            out = torch.empty_like(z)
        _lib.check(_lib.load().pcd_latent_persist_forward(h, z.data_ptr(), z.shape[0], tbias_row.data_ptr(), out.data_ptr(),
                                                          ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "latent_persist_forward")
        return out

    def forward_persist_guided(self, z, tbias_row, labels, w=None, out=None):
        """One launch: eps_u + w (eps_c - eps_u) per shape for ONE t shared by the batch (batch <= 32: a shape's conditional and
        null-class rows share a tile), or with w None the conditional eps (batch <= 64).  labels (B,) int32 on the device (a
        value outside the table reads the null row), w (1,) or (B,) fp32 on the device."""
        h, ws = self._persist_handle()
        cb = self.class_bias()
        if out is None:
            out = torch.empty_like(z)
        _lib.check(_lib.load().pcd_latent_persist_forward_guided(
            h, z.data_ptr(), z.shape[0], tbias_row.data_ptr(), cb.data_ptr(), cb.shape[0], cb.shape[0] - 1, labels.data_ptr(),
            0 if w is None else w.data_ptr(), 0 if w is None else int(w.numel() > 1), out.data_ptr(), ws.data_ptr(), ws.numel(),
            _lib.stream_ptr()), "latent_persist_forward_guided")
        return out

    def ddim_steps_persist_guided(self, z, x0, bias_table, rates, counter, nsteps, class_bias, labels, w):
        """`ddim_steps_persist` of a class-conditional run, still ONE launch: every step's bias row is bias_table[k] +
        class_bias[label] per shape, and with w (guided, batch <= 32) each shape's conditional and null-class rows share a tile
        and are combined in output.2's epilogue before the update."""
        h, ws = self._persist_handle()
        _lib.check(_lib.load().pcd_latent_persist_ddim_guided(
            h, z.data_ptr(), x0.data_ptr(), z.shape[0], bias_table.data_ptr(), bias_table.shape[1], class_bias.data_ptr(),
            class_bias.shape[0], class_bias.shape[0] - 1, labels.data_ptr(), 0 if w is None else w.data_ptr(),
            0 if w is None else int(w.numel() > 1), rates.data_ptr(), rates.shape[2], rates.shape[1], counter.data_ptr(), int(nsteps),
            ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "latent_persist_ddim_guided")

    def ddim_steps_persist(self, z, x0, bias_table, rates, counter, nsteps):
        """`nsteps` DDIM steps from table row counter[0] in ONE launch: z updated in place, x0 = the last step's x_0.
        rates (4, T, R) fp32 = (n, s, n_next, s_next)."""
        h, ws = self._persist_handle()
        _lib.check(_lib.load().pcd_latent_persist_ddim(h, z.data_ptr(), x0.data_ptr(), z.shape[0], bias_table.data_ptr(),
                                                       bias_table.shape[1], rates.data_ptr(), rates.shape[2], rates.shape[1],
                                                       counter.data_ptr(), int(nsteps), ws.data_ptr(), ws.numel(),
                                                       _lib.stream_ptr()), "latent_persist_ddim")

    def _ensure_packed(self):
        if self._packed is not None:
            return self._packed
        if (self.latent_dim, self.dim, self.time_dim) != (256, 512, 256):
            raise RuntimeError("the HIP latent denoiser is built for latent_dim=256, dim=512, time_dim=256 "
                               "(the configuration diffusion.py:362,380 instantiates)")
        dev = self._need_cuda()
        _lib.require_gpu()
        lib = _lib.load()
        lin, gn, ex = packing.pack_latent_unet(self.state_dict(), "")
        keep = {"freqs": packing.timestep_freqs(self.time_dim).to(dev)}
        for k, v in ex.items():
            keep[k] = _dev32(v, dev)
        desc = keep["desc"] = _lib.LatentDesc()
        f32 = self.precision == "fp32"
        for i, (w, b) in enumerate(lin):
            keep[f"w{i}"], keep[f"b{i}"] = (_dev32 if f32 else _dev16)(w, dev), _dev32(b, dev)
            desc.lin[i].w, desc.lin[i].b = keep[f"w{i}"].data_ptr(), keep[f"b{i}"].data_ptr()
            desc.lin[i].c, desc.lin[i].k = w.shape
        for i, (gm, bt) in enumerate(gn):
            keep[f"g{i}"], keep[f"be{i}"] = _dev32(gm, dev), _dev32(bt, dev)
            desc.gn_gamma[i], desc.gn_beta[i] = keep[f"g{i}"].data_ptr(), keep[f"be{i}"].data_ptr()
        if f32:
            self._handle = self._bind(desc, lib.pcd_latent_f32_create, lib.pcd_latent_f32_destroy, lib.pcd_latent_f32_workspace_bytes,
                                      lib.pcd_latent_f32_forward)
        else:
            self._handle = self._bind(desc, lib.pcd_latent_create, lib.pcd_latent_destroy, lib.pcd_latent_workspace_bytes,
                                      lib.pcd_latent_forward)
        self._packed = keep
        return keep

    def time_bias(self, t: torch.Tensor) -> torch.Tensor:
        """Hoisted time half of enc1 for each value of t: (len(t), 128) fp32."""
        return _time_embed(self, t, self.time_dim, 128)

    def class_bias(self) -> torch.Tensor:
        """Hoisted class half of enc1: the time columns applied to every row of `class_emb`, without the bias term
        (`time_bias` carries it), (num_classes + 1, 128) fp32.  Kept with the packed weights `time_bias` uses, so it is
        rebuilt whenever they are."""
        if not self.num_classes:
            raise RuntimeError("class_bias needs a class-conditional model (num_classes > 0)")
        pk = self._ensure_packed()
        if "class_bias" not in pk:
            emb = self.class_emb.weight.detach().to(torch.float32).contiguous()
            out = torch.empty(emb.shape[0], 128, dtype=torch.float32, device=self.device)
            _lib.check(_lib.load().pcd_linear_f32(emb.data_ptr(), emb.shape[0], self.time_dim, pk["e1w_t"].data_ptr(), None, 128,
                                                  out.data_ptr(), _lib.stream_ptr()), "linear_f32")
            pk["class_bias"] = out
        return pk["class_bias"]

    def forward(self, z: torch.Tensor, t: torch.Tensor, labels=None) -> torch.Tensor:
        self._need_cuda(z, t)
        if z.dim() != 2 or z.shape[1] != self.latent_dim:
            raise ValueError(f"z must be (B, {self.latent_dim}), got {tuple(z.shape)}")
        z = z.to(torch.float32).contiguous()
        tb = self.time_bias(t)
        if self.num_classes or labels is not None:
            lab = self.check_labels(labels, z.shape[0])
            cb = self.class_bias()
            _lib.check(_lib.load().pcd_embed_add_rows(tb.data_ptr(), cb.data_ptr(), lab.data_ptr(), z.shape[0], 128, cb.shape[0],
                                                      _lib.stream_ptr()), "embed_add_rows")
        return self.forward_with_bias(z, tb, 1)


def __getattr__(name):   # VAE3DLarge lives in vae.py; keep `networks.VAE3DLarge` importable like the reference
    if name in ("VAE3DLarge", "VAE3D"):
        from . import vae
        return getattr(vae, name)
    raise AttributeError(name)
