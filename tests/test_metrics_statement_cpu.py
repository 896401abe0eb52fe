"""tests/metrics_statement.py pinned to what already exists (the exact Chamfer of the oracle, the `metrics.npz` goldens, the oracle's
voxelize), and the record of how far its fp32 form lies from its fp64 form on the inputs of tests/test_gpu_metrics.py: the GPU
bounds of the stages that are not bit exact are 8 x these deviations (16 x for the cost stage), computed from the same helpers (tests/metrics_cases.py).

Recorded on one CPU (max over the elements of a stage and the pairs of a case; the last digits move with the CPU's vector width
and thread count, which is why the GPU test recomputes them where it runs instead of reading this table):
    pair entry, case      alpha      beta       row cost   cmax      EMD (relative)
    eps0.01               3.7e-08    6.5e-08    3.0e-09    2.3e-07   7.0e-07
    stops_differ          4.8e-08    6.5e-08    4.4e-07    1.9e-07   1.6e-07
    beta_decides          3.7e-08    9.2e-08    4.0e-08    1.1e-07   1.1e-07
    max_iter_first        3.7e-08    9.2e-08    4.0e-08    1.1e-07   1.1e-07
    never_stops           1.9e-08    6.5e-08    1.7e-08    1.1e-07   1.3e-07
Run with `-s` to see every figure."""
import math

import pytest
import torch
import torch.nn.functional as F

import metrics_cases as K
import metrics_statement as S
from oracle import torch_oracle as O


def test_fp64_statement_is_the_exact_chamfer_of_the_oracle(golden):
    g = golden("metrics.npz")
    a, b = torch.from_numpy(g["m_a"]), torch.from_numpy(g["m_b"])
    pairs = [(a[i], b[i]) for i in range(3)] + [(torch.from_numpy(g["units_x"])[0], torch.from_numpy(g["units_y"])[0]),
                                                  (a[0, :7], b[0, :200])] + [K.matched(300, 300, 5), K.gaussian(130, 77, 6)]
    for x, y in pairs:
        got, want = S.pair(x, y, torch.float64, False)["chamfer"], O.chamfer_distance_exact(x, y, 1)
        assert got.dtype == want.dtype == torch.float64
        assert abs(float(got) - float(want)) <= 1e-13 * float(want)                  # fp64 rounding of two means of up to ~1e3 terms
    # the batch form of the oracle is the mean of the per-pair values when the sizes are equal
    per = torch.stack([S.pair(a[i], b[i], torch.float64, False)["chamfer"] for i in range(3)])
    assert abs(float(per.mean()) - float(O.chamfer_distance_exact(a, b, 1))) <= 1e-15
    assert float(S.pair(a[0], a[0], torch.float32, False)["chamfer"]) == 0.0


def test_statement_against_the_metric_goldens(golden):
    g = golden("metrics.npz")
    a, b = torch.from_numpy(g["m_a"]), torch.from_numpy(g["m_b"])
    assert torch.equal(S.normalize(a), torch.from_numpy(g["m_norm_a"]))                 # fp32, bit exact
    assert torch.equal(S.normalize(a), O.normalize_to_cube(a))
    assert torch.equal(S.pair(a[1], b[1], torch.float64, False)["an"], torch.from_numpy(g["m_norm_a"])[1])
    # the goldens' cost matrix is the reference's matmul-form cdist: 2e-3 relative, as tests/test_gpu_kernels.py holds the kernels
    ux, uy = torch.from_numpy(g["units_x"]), torch.from_numpy(g["units_y"])
    for dt in (torch.float64, torch.float32):
        got = float(S.sinkhorn(S.normalize(ux), S.normalize(uy), dtype=dt)["emd"].mean())
        assert abs(got - float(g["units_emd_sinkhorn"])) < 2e-3 * float(g["units_emd_sinkhorn"])
        got = float(S.sinkhorn(S.normalize(a), S.normalize(b), dtype=dt)["emd"].mean())        # batch-joint: one C.max(), one stop
        assert abs(got - float(g["m_emd_sinkhorn_batch"])) < 2e-3 * float(g["m_emd_sinkhorn_batch"])
        r = S.pair(a[0], b[0], dt)
        w = g["m_triple_sinkhorn0"]
        assert abs(float(r["chamfer"]) * 1e3 - w[0]) < 0.1 and abs(float(r["emd"]) - w[1]) < 2e-3 * w[1] and float(r["bce"]) == w[2]
    # the cloud 0 of the batch on its own is the per-pair form: own cmax, which is not the batch's
    joint, own = S.sinkhorn(S.normalize(a), S.normalize(b)), S.pair(a[0], b[0])
    assert float(joint["cmax"]) >= float(own["cmax"]) and joint["alpha"].shape == (3, 256) and own["alpha"].shape == (256,)
    assert len(own["iters"]) == own["stop"] and torch.equal(own["iters"][-1]["beta"], own["beta"])


def test_voxel_statement_is_the_oracle_on_every_edge(golden):
    g = golden("metrics.npz")
    a = torch.from_numpy(g["m_a"])
    edge = torch.tensor([[-1.0, 1.0, 0.0], [1.5, -1.5, 100.0], [-100.0, float("nan"), 0.999999], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0],
                         [-1.0000001, 0.9999999, 1.0000001], [2.0 / 31 - 1, 2.0 / 31 - 1 - 1e-7, 0.0]])
    for pts in (a[0], edge):
        assert torch.equal(S.voxelize(pts), O.voxelize(pts)[0])
    idx = S.voxel_indices(edge)
    assert idx[0].tolist() == [0, 31, 15] and idx[1].tolist() == [31, 0, 31] and idx[2].tolist() == [0, 0, 30]   # NaN -> 0
    occ = torch.nonzero(S.voxelize(a[0]).reshape(-1))[:, 0]
    assert torch.equal(occ.to(torch.int32), torch.from_numpy(g["m_vox_a_idx"]))
    k = int((S.voxelize(a[0]) != S.voxelize(a[1])).sum())
    assert float(S.pair(a[0], a[1], torch.float64, False)["bce"]) == 100.0 * k / 32768


@pytest.mark.parametrize("name", list(K.PAIR_SINKHORN_CASES))
def test_fp32_statement_next_to_fp64_on_the_gpu_inputs(name):
    """The numbers the GPU bounds are made of.  The bands asserted here are the ones the fp32 arithmetic explains: a dual is
    epsilon x (a log-sum-exp of ~n terms of size <= 1/epsilon), so ~|dual| 2^-24 sqrt-ish growth keeps it below 2e-7; the EMD is a
    sum of products of three fp32 factors: below 2e-6 relative."""
    _, _, epsilon, thresh, max_iter = K.pair_sinkhorn_case(name)
    runs = K.pair_sinkhorn_statements(name)
    worst = {}
    for i, (r64, r32) in enumerate(runs):
        assert r64["stop"] == r32["stop"] <= max_iter
        for key in ("alpha", "beta", "row_cost", "cmax"):
            worst[key] = max(worst.get(key, 0.0), K.deviation(r32, r64, key))
        worst["emd"] = max(worst.get("emd", 0.0), K.deviation(r32, r64, "emd", relative=True))
        print(name, i, "stop", r64["stop"], {k: "%.2e" % K.deviation(r32, r64, k) for k in ("alpha", "beta", "row_cost", "cmax")},
              "emd rel %.2e" % K.deviation(r32, r64, "emd", True), "chamfer %.2e" % K.deviation(r32, r64, "chamfer"))
        assert K.deviation(r32, r64, "chamfer") < 5e-7                               # the Chamfer bound of 2e-6 leaves 4 x
        assert torch.equal(r32["an"], r64["an"]) and torch.equal(r32["vox_a"], r64["vox_a"]) and float(r32["bce"]) == float(r64["bce"])
    print(name, "case", {k: "%.2e" % v for k, v in worst.items()})
    assert 0 < worst["alpha"] < 2e-7 and 0 < worst["beta"] < 2e-7 and 0 < worst["cmax"] < 6e-7 and 0 < worst["emd"] < 2e-6
    assert 8 * worst["emd"] <= 2e-5                                                  # the EMD bound may not exceed 2e-5 relative


def test_the_stop_cases_are_decided_by_a_factor_of_at_least_one_and_a_half():
    """fp32 rounding moves an error by ~1e-7 at most; every error that decides a stop lies a factor >= 1.5 from thresh in fp64."""
    stops = {}
    for name in K.PAIR_SINKHORN_CASES:
        _, _, epsilon, thresh, max_iter = K.pair_sinkhorn_case(name)
        runs = K.pair_sinkhorn_statements(name)
        stops[name] = [r64["stop"] for r64, _ in runs]
        for r64, _ in runs:
            assert K.stop_margin(r64, thresh) >= 1.5, (name, K.stop_margin(r64, thresh))
    assert stops["eps0.01"] == [3, 3, 3, 3, 3]
    assert stops["stops_differ"] == [3, 4, 4, 4]                                     # one call, two stopping iterations
    assert stops["max_iter_first"] == [2, 2] and stops["stops_differ"][1] > 2        # max_iter ends it before the errors do
    assert stops["never_stops"] == [100, 100]
    # beta_decides: after iteration 1 of pair 0 only beta's error is above thresh
    _, _, _, thresh, _ = K.pair_sinkhorn_case("beta_decides")
    first = K.pair_sinkhorn_statements("beta_decides")[0][0]["iters"][0]
    assert float(first["err_alpha"]) * 1.5 <= thresh and float(first["err_beta"]) >= 1.5 * thresh
    assert stops["beta_decides"] == [2, 2]


@pytest.mark.parametrize("n,m", K.JOINT_SIZES)
def test_fp32_stage_statements_next_to_fp64_on_the_joint_inputs(n, m):
    x, y, dual_q, dual_p = K.joint_case(n, m)
    for epsilon in K.JOINT_EPSILONS:
        d = K.joint_stage_deviations(n, m, epsilon)
        print(n, m, epsilon, {k: "%.2e" % v for k, v in d.items()})
        assert 0 < d["dual"] < (2e-7 if epsilon < 0.1 else 2e-6) and 0 < d["row_cost"] and 0 < d["cost"] < 2e-6


def test_bce_statement_cases():
    """`F.binary_cross_entropy` in fp64 is the yardstick of pcd_binary_bce_mean; the fp32 torch call's deviation is its bound / 8."""
    for n in K.BCE_LENGTHS:
        for kind in K.BCE_KINDS:
            x, t, exact = K.bce_case(n, kind)
            want = float(F.binary_cross_entropy(x.double(), t.double()))
            dev = abs(float(F.binary_cross_entropy(x, t)) - want)
            print(n, kind, want, "%.2e" % dev)
            if exact is not None:
                assert want == exact or abs(want - exact) <= 2.0 ** -50 * exact
            assert math.isfinite(want) and dev <= 2.0 ** -22 * max(want, 1.0)
