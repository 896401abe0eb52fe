"""numpy statement of the packed weight buffers of the register-resident chains (csrc/widechain.hip, wideffn.hip, sab_tail.hip): stage images of
1-KiB pieces in MFMA fragment order, then rows of fp32 parameters.

A fragment block is w[row0 : row0 + 32 ntile, k0 : k0 + 16 nq] with the rows at or past `row_limit` zero, cut into [ntile][32 rows][nq][2 halves][8] and
ordered (tile, k-step, half, row, element): piece (t nq + q) 64 + lane holds the 8 halfs W[row0 + 32 t + (lane & 31)][k0 + 16 q + 8 (lane >> 5) .. + 7].

A buffer is a list of parts in memory order:
    ("frag", weight, row0, row_limit, k0, ntile, nq)     weight: index / name into the packer's fp16 matrices
    ("zero", nbytes)
    ("f32", source, n)                                    source: index / name into the packer's fp32 vectors, its first n floats
Weights and parameters are addressed as the packer's own arguments are: `w[i]` / `b[i]` by index, the attention block's by descriptor field."""
import numpy as np

STAGE = 32768          # a stage image of the 256-wide chains: 32 pieces


def fragment_block(w, row0, row_limit, k0, ntile, nq):
    """-> the block's bytes (uint8, 1024 ntile nq of them)"""
    w = np.asarray(w, np.float16)
    blk = np.zeros((32 * ntile, 16 * nq), np.float16)
    n = max(0, min(row_limit, w.shape[0], row0 + 32 * ntile) - row0)
    blk[:n] = w[row0:row0 + n, k0:k0 + 16 * nq]
    return np.ascontiguousarray(blk.reshape(ntile, 32, nq, 2, 8).transpose(0, 2, 3, 1, 4)).view(np.uint8).reshape(-1)


def assemble(parts, weights, params):
    """the bytes of a buffer (uint8)"""
    out = []
    for p in parts:
        if p[0] == "frag":
            out.append(fragment_block(weights[p[1]], *p[2:]))
        elif p[0] == "zero":
            out.append(np.zeros(p[1], np.uint8))
        else:
            v = np.ascontiguousarray(np.asarray(params[p[1]], np.float32)[:p[2]])
            assert v.size == p[2]
            out.append(v.view(np.uint8))
    return np.concatenate(out)


def size(parts):
    return sum(1024 * p[5] * p[6] if p[0] == "frag" else p[1] if p[0] == "zero" else 4 * p[2] for p in parts)


def _pass256(w, row0, row_limit, k0):
    """one 256-channel output pass over 256 k: four images of 256 channels x 64 k"""
    return [("frag", w, row0, row_limit, k0 + 64 * kt, 8, 4) for kt in range(4)]


def pw_wide(chain):
    """pcd_pw_wide_pack.  E3: enc3.conv1 [256][256], conv2 [256][256], conv3 [512][256] (two passes); D2: dec2.conv1 [256][512] (two K halves), conv2
    [256][256], conv3 [128][256] (padded to 256 channels).  Four passes of four images, then one bias row of 256 floats per pass."""
    if chain == 0:
        return (_pass256(0, 0, 256, 0) + _pass256(1, 0, 256, 0) + _pass256(2, 0, 512, 0) + _pass256(2, 256, 512, 0)
                + [("f32", 0, 256), ("f32", 1, 256), ("f32", 2, 512)])
    return (_pass256(0, 0, 256, 0) + _pass256(0, 0, 256, 256) + _pass256(1, 0, 256, 0) + _pass256(2, 0, 128, 0)
            + [("zero", 1024), ("f32", 0, 256), ("f32", 1, 256), ("f32", 2, 128), ("zero", 512)])      # (the first K half has no epilogue)


def _segment(w, c, row0, k0, k):
    """a segment of the ends: K = k input channels from column k0 on, C = c output channels from row row0 on.  An image is always 32 pieces:
    256 channels x 64 k or 128 channels x 128 k"""
    nt, nq = c // 32, 1024 // c
    return [("frag", w, row0, 1 << 30, k0 + 16 * nq * i, nt, nq) for i in range(k // (16 * nq))]


def pw_wide_ends(chain, hilo):
    """pcd_pw_wide_ends_pack.  E23: enc2.conv1-3 + enc3.conv1-3; D21: dec2.conv1-3 + dec1.conv1.  With `hilo` the narrow layer (enc2.conv3 / dec1.conv1)
    is [C][hi K | lo K]: all hi K passes, then all lo passes.  The images in execution order, then the layers' biases one after the other."""
    if chain == 0:
        parts = _segment(0, 128, 0, 0, 128) + _segment(1, 128, 0, 0, 128) + _segment(2, 256, 0, 0, 128)
        if hilo:
            parts += _segment(2, 256, 0, 128, 128)
        parts += _segment(3, 256, 0, 0, 256) + _segment(4, 256, 0, 0, 256) + _segment(5, 256, 0, 0, 256) + _segment(5, 256, 256, 0, 256)
        return parts + [("f32", i, c) for i, c in enumerate((128, 128, 256, 256, 256, 512))]
    parts = _segment(0, 256, 0, 0, 256) + _segment(0, 256, 0, 256, 256) + _segment(1, 256, 0, 0, 256) + _segment(2, 128, 0, 0, 256)
    parts += _segment(3, 128, 0, 0, 256)
    if hilo:
        parts += _segment(3, 128, 0, 256, 256)
    return parts + [("f32", i, c) for i, c in enumerate((256, 256, 128, 128))]


def ln_linear(passes):
    """pcd_pw_wide_ln_linear_pack: w [256 passes][256] as `passes` output passes | b [256 passes] | gamma [256] | beta [256]"""
    parts = []
    for i in range(passes):
        parts += _pass256("w", 256 * i, 256 * passes, 0)
    return parts + [("f32", "b", 256 * passes), ("f32", "ln_g", 256), ("f32", "ln_b", 256)]


def wide_ffn():
    """pcd_wide_ffn_pack: per 128-channel slab of the hidden layer, W1's 128 rows x K 256 as two images ([4 tiles][8 k-steps], 128 k each) and
    W2's 256 rows x the slab's 128 k as two images ([8 tiles][4 k-steps], 64 k each); then b1 [1024] | b2 [256] | gamma [256] | beta [256]"""
    parts = []
    for slab in range(8):
        parts += [("frag", "w1", 128 * slab, 1024, 128 * j, 4, 8) for j in range(2)]
        parts += [("frag", "w2", 0, 256, 128 * slab + 64 * j, 8, 4) for j in range(2)]
    return parts + [("f32", "b1", 1024), ("f32", "b2", 256), ("f32", "ln_g", 256), ("f32", "ln_b", 256)]


def sab_tail(c):
    """pcd_sab_tail_pack at C = c.  The tail: stage images of 32 KiB (C 128) / 16 KiB (C 64): W_out ([C / 32 tiles][C / 16 k-steps], the rest of
    the image zero), then per 64-wide chunk of the 4C hidden channels [W1 chunk: 2 tiles x C / 16 k-steps | W2 chunk: C / 32 tiles x 4 k-steps];
    b_out | ln2 gamma | ln2 beta | b_ff2 | b_ff1 [4C].  The head behind it: W_in as three C-wide passes (images of C x C); b_in [3C] | ln1 gamma | ln1 beta."""
    nt, ks, stage = c // 32, c // 16, {128: 32768, 64: 16384}[c]
    parts = [("frag", "w_out", 0, c, 0, nt, ks), ("zero", stage - 1024 * nt * ks)]
    for ch in range(c // 16):
        parts += [("frag", "w_ff1", 64 * ch, 4 * c, 0, 2, ks), ("frag", "w_ff2", 0, c, 64 * ch, nt, 4)]
    parts += [("f32", "b_out", c), ("f32", "ln2_g", c), ("f32", "ln2_b", c), ("f32", "b_ff2", c), ("f32", "b_ff1", 4 * c)]
    parts += [("frag", "w_in", c * i, 3 * c, 0, nt, ks) for i in range(3)]
    return parts + [("f32", "b_in", 3 * c), ("f32", "ln1_g", c), ("f32", "ln1_b", c)]
