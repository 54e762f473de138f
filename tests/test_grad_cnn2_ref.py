"""CPU: tests/grad_cnn2_ref.py against torch's fp64 autograd on the same fp32-rounded
model under grad_cnn2_ref.torch_gate.  Asserted of the inputs: both forwards take the same
side of every ReLU and select the same element of every pool window with a positive maximum."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import cnn2_ref
import grad_cnn2_ref as R

MAX_NORM = 100.0


def torch_step(shape, ww, X, y):
    ci, h, w, k, pad = shape[:5]
    p = [torch.from_numpy(a.astype(np.float32).astype(np.float64)).requires_grad_() for a in cnn2_ref.split(shape, ww)]
    x = torch.from_numpy(X.astype(np.float64).reshape(len(X), ci, h, w))
    P1 = Fn.conv2d(x, p[0], p[1], 1, pad)
    P2 = Fn.conv2d(Fn.max_pool2d(Fn.relu(P1), 2, 2), p[2], p[3], 1, pad)
    out = Fn.linear(Fn.max_pool2d(Fn.relu(P2), 2, 2).reshape(len(X), -1), p[4], p[5])
    loss = Fn.cross_entropy(out, torch.from_numpy(y.astype(np.int64)))
    loss.backward()
    norm = float(torch.nn.utils.clip_grad_norm_(p, MAX_NORM))
    return -np.concatenate([t.grad.numpy().ravel() for t in p]), float(loss.detach()), norm, P1.detach().numpy(), P2.detach().numpy()


@pytest.mark.parametrize("shape,count,seed,grow", [((3, 6, 6, 3, 1, 5, 17, 3), 5, 21, 1.0),
                                                   ((3, 8, 6, 2, 1, 18, 36, 2), 5, 22, 8.0),
                                                   (cnn2_ref.LFW, 4, 23, 1.0)])
def test_restatement_against_torch(shape, count, seed, grow):
    ww, X, y = cnn2_ref.make_case(shape, count, seed)
    ww = ww * grow  # grow > 1: scaled until torch's norm exceeds MAX_NORM
    want, tloss, tnorm, T1, T2 = torch_step(shape, ww, X, y)
    assert (tnorm > MAX_NORM) == (grow > 1.0)
    m = R.maps(shape, ww, X)
    for mine, theirs in ((m["P1"], T1), (m["P2"], T2)):
        assert np.array_equal(mine > 0, theirs > 0)
        relu = np.maximum(theirs, 0.0)
        live = cnn2_ref.pool(relu) > 0
        assert np.array_equal(R.select(np.maximum(mine, 0))[live], R.select(relu)[live])
    delta, loss, norm = R.step(shape, X, y, ww, max_norm=MAX_NORM)
    scale, gate = R.scale(shape, X, ww), R.torch_gate(shape, count)
    dev = float(np.max(np.abs(delta - want)) / scale)
    print(shape, "deviation", dev, "gate", gate, "norm", norm, tnorm, "loss", loss, tloss)
    assert dev <= gate
    assert abs(norm - tnorm) <= gate * max(tnorm, scale)
    assert abs(loss - tloss) <= gate * max(abs(tloss), 1.0)
