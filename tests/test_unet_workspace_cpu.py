"""pcd_unet_workspace_bytes covers everything pcd_unet_forward puts into the workspace, also for shapes of a few points."""
import pytest


@pytest.mark.parametrize("batch,n", [(1, 1), (3, 2), (2, 15), (256, 1), (2, 16), (3, 100)])
def test_point_unet_workspace_holds_the_pooled_product_slabs(batch, n):
    """For batch <= 256 the forward writes the split-K slabs of the pooled product (slabs x batch x 1024 floats) into one of its activation buffers and
    reads them back beside the pooled maxima (batch x 4096 floats) and the per-shape bias rows (batch x 1024 floats) they produce; all three must fit
    next to the activations, which at n < 16 points per shape are smaller than the slabs (the forward once wrote 10 KB past a (1, 1) workspace)."""
    from shapegen_amd import _lib
    lib = _lib.load()
    slabs = lib.pcd_skinny_slabs(4096, 1024)
    assert slabs >= 1
    m = batch * n
    activations = m * (128 + 256 + 512 + 1024 + 2048) * 2            # x1 .. x4 and the widest scratch row, fp16
    need = activations + max(m * 1024 * 2, slabs * batch * 1024 * 4) + batch * 4096 * 4 + batch * 1024 * 4
    assert lib.pcd_unet_workspace_bytes(batch, n) >= need
