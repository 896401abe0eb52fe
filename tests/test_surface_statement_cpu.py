"""tests/surface_statement.py against cases worked out by hand.  No GPU."""
import math

import torch

import surface_statement as S

A = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
B = torch.tensor([[0.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
NA = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
NB = torch.tensor([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])


def test_three_points_against_two():
    """a0 -> b0 (1), a1 -> b1 (1), a2 -> b1 (2); b0 -> a0 (1), b1 -> a1 (1: a0 and a2 are at 2)."""
    for dt in (torch.float32, torch.float64):
        r = S.row(A, B, NA, NB, (1.0, 1.5), dt)
        assert r["d2_a"].tolist() == [1.0, 1.0, 2.0] and r["index_a"].tolist() == [0, 1, 1]
        assert r["d2_b"].tolist() == [1.0, 1.0] and r["index_b"].tolist() == [0, 1]
        assert r["within"] == [(2, 2), (3, 2)]
        row = r["row"]
        assert row.dtype == dt and row.shape == (S.BASE + 6,)
        acc = torch.tensor((2 + math.sqrt(2.0)) / 3, dtype=torch.float64).to(dt)
        want = {S.ACC: acc, S.COMP: 1.0, S.CHAMFER_L1: (acc + 1) / 2, S.ACC2: torch.tensor(4 / 3, dtype=torch.float64).to(dt), S.COMP2: 1.0,
                S.HAUSDORFF: torch.tensor(math.sqrt(2.0), dtype=torch.float64).to(dt),
                S.NC_A: torch.tensor(2 / 3, dtype=torch.float64).to(dt), S.NC_B: 0.5}     # |n.n'| = 1, 0, 1 over a; 1, 0 over b
        for col, v in want.items():
            assert float(row[col]) == float(v), (dt, col)
        assert float(row[S.CHAMFER_L2]) == float(row[S.ACC2] + 1)
        assert float(row[S.NC]) == float((row[S.NC_A] + 0.5) / 2)
        p = torch.tensor(2.0, dtype=dt) / torch.tensor(3.0, dtype=dt)                        # tau = 1: 2 of 3 in a, 2 of 2 in b
        assert float(row[S.BASE]) == float(p) and float(row[S.BASE + 1]) == 1.0
        assert float(row[S.BASE + 2]) == float((2 * p * 1) / (p + 1)) and abs(float(row[S.BASE + 2]) - 0.8) < 1e-6
        assert row[S.BASE + 3:].tolist() == [1.0, 1.0, 1.0]                                  # tau = 1.5: all of both
    # without normals the NC columns are NaN and the others are the same
    bare = S.row(A, B, None, None, (1.0, 1.5))["row"]
    full = S.row(A, B, NA, NB, (1.0, 1.5))["row"]
    nc = [S.NC_A, S.NC_B, S.NC]
    assert torch.isnan(bare[nc]).all()
    keep = [c for c in range(bare.shape[0]) if c not in nc]
    assert torch.equal(bare[keep], full[keep])


def test_a_tie_goes_to_the_lowest_index():
    q = torch.zeros(1, 3)
    t = torch.tensor([[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    d2, index = S.nearest(q, t)
    assert d2.tolist() == [1.0] and index.tolist() == [1]                    # targets 1, 2, 3, 4 are all at distance 1
    d2, index = S.nearest(q, t.flip(0))
    assert d2.tolist() == [1.0] and index.tolist() == [0]


def test_a_point_exactly_on_a_threshold_counts():
    q = torch.zeros(1, 3)
    t = torch.tensor([[0.25, 0.0, 0.0]])
    below = float(torch.nextafter(torch.tensor(0.25), torch.tensor(0.0)))
    r = S.row(q, t, None, None, (0.25, below, 0.5))
    assert r["d2_a"].tolist() == [0.0625] and r["within"] == [(1, 1), (0, 0), (1, 1)]
    assert r["row"][S.BASE:].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0]     # FSCORE 0 where P + R = 0
    # 0.1 is not a dyadic number: the comparison is against the fp32 product tau * tau
    tau = torch.tensor(0.1)
    d = S.sqrt(tau * tau, torch.float32)
    on = torch.tensor([[float(d), 0.0, 0.0]])
    d2, _ = S.nearest(q, on)
    assert S.counts(d2, d2, (0.1,)) == [(int(d2[0] <= tau * tau),) * 2]


def test_non_finite_points_have_no_neighbours_and_are_nobodys():
    nan, inf = float("nan"), float("inf")
    q = torch.tensor([[0.0, 0.0, 0.0], [nan, 0.0, 0.0], [1.0, 0.0, 0.0]])
    t = torch.tensor([[inf, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, nan, 0.0]])
    d2, index = S.nearest(q, t)
    assert index.tolist() == [1, -1, 1] and d2[0] == 9.0 and d2[2] == 4.0 and torch.isnan(d2[1])
    d2, index = S.nearest(q, t[[0, 2]])                                        # no finite target at all
    assert index.tolist() == [-1, -1, -1] and torch.isnan(d2).all()
    d2, index = S.nearest(q, t[:0])
    assert index.tolist() == [-1, -1, -1] and torch.isnan(d2).all()
    assert torch.isnan(S.row(q, t[1:2], None, None, (0.1,))["row"]).all()      # a NaN coordinate in a: no row
    assert torch.isnan(S.row(q[:1], t, None, None, (0.1,))["row"]).all()       # an infinite one in b
    assert torch.isnan(S.row(q[:0], t[1:2], None, None, (0.1,))["row"]).all()  # an empty cloud


def test_iou_counts():
    a = torch.tensor([0.0, 1.0, 1.0, 0.6, 0.5, 0.0])
    b = torch.tensor([0.0, 1.0, 0.0, 0.7, 0.9, 0.0])
    assert float(S.iou(a, b)) == float(torch.tensor(2.0) / torch.tensor(4.0))            # 0.5 itself is not occupied
    assert float(S.iou(a, b, 0.65)) == float(torch.tensor(1.0) / torch.tensor(4.0))
    assert torch.isnan(S.iou(torch.zeros(8), torch.zeros(8)))
    assert float(S.iou(a, a)) == 1.0 and float(S.iou(a, 1 - (a > 0.5).float())) == 0.0
