"""tests/cnn2_ref.py against torch on the CPU: the restated logits lie within the
bound E_c of torch's fp64 forward pass, and every sample the restatement does
not flag has the prediction of torch's fp32 forward pass."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import cnn2_ref


def torch_forward(shape, ww, X, dtype):
    ci, h, w, k, pad = shape[:5]
    w1, b1, w2, b2, fw, fb = (torch.from_numpy(a.astype(np.float32)).to(dtype) for a in cnn2_ref.split(shape, ww))
    x = torch.from_numpy(X.reshape(len(X), ci, h, w)).to(dtype)
    x = Fn.max_pool2d(Fn.relu(Fn.conv2d(x, w1, b1, 1, pad)), 2, 2)
    x = Fn.max_pool2d(Fn.relu(Fn.conv2d(x, w2, b2, 1, pad)), 2, 2)
    return Fn.linear(x.reshape(len(X), -1), fw, fb).numpy()


@pytest.mark.parametrize("shape,nv,seed", [(cnn2_ref.LFW, 16, 7), ((3, 9, 8, 3, 1, 5, 17, 3), 64, 11),
                                           ((2, 8, 6, 2, 1, 18, 36, 2), 64, 12)])
def test_restatement_against_torch(shape, nv, seed):
    ww, X, _ = cnn2_ref.make_case(shape, nv, seed)
    lg, E = cnn2_ref.forward(shape, ww, X)
    flag = cnn2_ref.near_ties(lg, E)
    l64, l32 = torch_forward(shape, ww, X, torch.float64), torch_forward(shape, ww, X, torch.float32)
    fin = np.isfinite(lg).all(axis=1)
    diff = np.abs(lg.astype(np.float64) - l64)
    print(shape, "flagged", int(flag.sum()), "of", nv, "max |logit - fp64|", diff.max(), "min E_c", E.min(),
          "max |fp32 torch - fp64|", np.abs(l32 - l64).max())
    assert fin.all() and (diff[fin] <= E[fin]).all()
    assert np.array_equal(np.argmax(lg, axis=1)[~flag], np.argmax(l32, axis=1)[~flag])
    assert 2 * int(flag.sum()) <= nv
