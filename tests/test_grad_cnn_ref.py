"""CPU: tests/grad_cnn_ref.py against the torch goldens of the reference's
MNISTCNNModel (tests/golden/gen_grad_cnn_goldens.py) under the derived gate
grad_cnn_ref.torch_gate, in units of the norm-wise scale."""
import pytest

import numpy as np

import cnn_ref
import grad_cnn_ref as R


@pytest.mark.parametrize("name", R.golden_names())
def test_restatement_against_torch(name):
    c = R.load_golden(name)
    p = c["p"]
    delta, loss, norm = R.step(cnn_ref.MNIST, c["X"], c["y"], c["ww"], c["idx"])
    scale = R.scale(cnn_ref.MNIST, c["X"], c["ww"], c["idx"])
    gate = R.torch_gate(cnn_ref.MNIST, p["count"])
    dev = float(np.max(np.abs(delta - c["delta"])) / scale)
    print(name, "deviation", dev, "recorded", p["ref_deviation"], "gate", gate, "norm", norm, c["norm"])
    assert gate == p["gate"] and scale == p["scale"]
    assert p["ref_deviation"] <= gate and dev <= gate
    assert abs(norm - c["norm"]) <= gate * max(c["norm"], scale)
    assert abs(loss - c["loss"]) <= gate * max(abs(c["loss"]), 1.0)
    assert (norm > 100.0) == (name == "grad_cnn_clip")
