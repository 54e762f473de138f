"""Writes tests/golden/cnnc_cifar_logits.npz: torch's fp32 logits and predictions
of the reference's own CIFARCNNModel (ML/Pytorch/cifar_cnn_model.py) on the
model and the 64 images of cnnc_ref.make_case(CIFAR, 64, SEED).  The inputs are
rebuilt from the seed by the test, so no weights are stored.  Run on the CPU:

    python tests/golden/gen_cnnc_goldens.py <reference>/ML/Pytorch

It asserts, with cnnc_ref's near-tie count against torch's logits, that every
unflagged sample has torch's prediction and that at most half are flagged (a
condition of the test: a seed that exceeds it is replaced here, never the cap).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cnnc_ref  # noqa: E402

SEED, NV = 3501, 64


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    from cifar_cnn_model import CIFARCNNModel
    ww, X, _ = cnnc_ref.make_case(cnnc_ref.CIFAR, NV, SEED)
    model = CIFARCNNModel()
    with torch.no_grad():
        for p, layer in zip(model.parameters(), model.reshape(ww)):
            p.copy_(layer)
        logits = model(torch.from_numpy(X.reshape(NV, 3, 32, 32))).numpy()
    pred = np.argmax(logits, axis=1)
    lg, E = cnnc_ref.forward(cnnc_ref.CIFAR, ww, X)
    flag = cnnc_ref.near_ties(lg, E)
    assert np.array_equal(np.argmax(lg, axis=1)[~flag], pred[~flag])
    share = float(flag.mean())
    assert share <= 0.5, share
    np.savez(os.path.join(HERE, "cnnc_cifar_logits.npz"), seed=SEED, logits=logits.astype(np.float32),
             pred=pred.astype(np.int32), share=share,
             max_abs_diff=float(np.abs(lg.astype(np.float64) - logits).max()))
    print("flagged share %.4f, max |logit - torch| %.3e" % (share, np.abs(lg - logits).max()))


if __name__ == "__main__":
    main(sys.argv[1])
