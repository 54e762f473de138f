"""The numpy restatement of the gradient step (tests/grad_ref.py) against every
golden the reference's own code produced (tests/golden/gen_grad_goldens.py),
normalised by the norm-wise scale.  No GPU.

logistic  1e-9 x scale, scale = max_j [alpha (sum_i |x_ij| / batch_size + lammy
          |w_j|) + |noise_j|]: both sides are fp64
softmax   (d_in + count + 8) 2^-24 x scale, scale = max(max_k sum_i |x_ik| /
          count, 1): the golden is torch fp32
"""
import numpy as np
import pytest

import grad_cases as GC
import grad_ref as R


@pytest.mark.parametrize("name", GC.names("logistic"))
def test_logistic_restatement(name):
    c = GC.load(name)
    p = c["p"]
    delta, loss = R.logistic(c["X"], c["y"], c["ww"], c["idx"], p["batch"], p["alpha"], p["lammy"],
                             c["noise"])
    scale = R.logistic_scale(c["X"], c["ww"], c["idx"], p["batch"], p["alpha"], p["lammy"],
                             c["noise"])
    dev = float(np.max(np.abs(delta - c["delta"])) / scale)
    print(name, "deviation", dev, "recorded", p["ref_deviation"])
    assert np.isfinite(delta).all()
    assert dev <= GC.FP64_GATE
    assert abs(loss - c["loss"]) <= GC.FP64_GATE * max(abs(c["loss"]), 1.0)


@pytest.mark.parametrize("name", GC.names("softmax"))
def test_softmax_restatement(name):
    c = GC.load(name)
    p = c["p"]
    delta, loss, norm = R.softmax(c["X"], c["y"], c["ww"], c["idx"], p["C"])
    scale = R.softmax_scale(c["X"], c["idx"])
    gate = GC.softmax_gate(p["din"], p["count"])
    dev = float(np.max(np.abs(delta - c["delta"])) / scale)
    print(name, "deviation", dev, "gate", gate, "recorded", p["ref_deviation"])
    assert dev <= gate
    # the loss and the norm are fp32 scalars of the reference
    assert abs(loss - c["loss"]) <= gate * max(abs(c["loss"]), 1.0)
    assert abs(norm - c["norm"]) <= gate * max(c["norm"], scale)
    if "xscale" in p:
        assert c["norm"] > 100.0 and norm > 100.0  # the clip acts


def test_the_cases_the_issue_names_exist():
    lg = {(GC.manifest()[n]["count"], GC.manifest()[n]["d"]) for n in GC.names("logistic")}
    assert {(1, 1), (10, 25), (256, 25), (257, 33), (700, 100), (600, 25), (200, 25)} <= lg
    sm = {(p["count"], p["din"], p["C"]) for p in (GC.manifest()[n] for n in GC.names("softmax"))}
    assert {(1, 1, 2), (10, 784, 10), (7, 24, 2), (16, 100, 16), (257, 70, 3), (5, 8742, 12)} <= sm


def test_quantize_is_gos_int64():
    v = np.array([1.23456789, -1.99999, 0.0, -0.0, 1e11, np.nan, np.inf, -np.inf, 1e300])
    q = R.quantize(v, 4)
    assert q.tolist() == [12345, -19999, 0, 0, 10 ** 15, R.INT64_MIN, R.INT64_MIN, R.INT64_MIN,
                          R.INT64_MIN]


def test_tiles_and_divisor():
    # a batch past one tile sums tile by tile; batch_size is the divisor, not the count
    rng = np.random.default_rng(7)
    X = rng.standard_normal((300, 5))
    y = rng.choice([-1.0, 1.0], 300)
    w = rng.standard_normal(5)
    d1, _ = R.logistic(X, y, w, None, 300, 1e-2, 0.0)
    d2, _ = R.logistic(X, y, w, None, 600, 1e-2, 0.0)
    assert np.allclose(d1, 2.0 * d2, rtol=1e-15, atol=0)
    t = y * (X @ w)
    plain = -1e-2 * ((X * (-y / (1.0 + np.exp(t)))[:, None]).sum(0) / 300.0)
    assert np.max(np.abs(d1 - plain)) <= 1e-15
