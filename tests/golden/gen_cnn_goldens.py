"""Writes tests/golden/cnn_mnist_logits.npz: torch's fp32 logits and predictions
of the reference's own MNISTCNNModel (ML/Pytorch/mnist_cnn_model.py) on the
model and the 64 images of cnn_ref.make_case(MNIST, 64, SEED).  The inputs are
rebuilt from the seed by the test, so no weights are stored.  Run on the CPU:

    python tests/golden/gen_cnn_goldens.py <reference>/ML/Pytorch

It asserts, with cnn_ref's near-tie count against torch's logits, that every
unflagged sample has torch's prediction and that at most half are flagged (a
condition of the test: a seed that exceeds it is replaced here, never the cap).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cnn_ref  # noqa: E402

SEED, NV = 2901, 64


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    from mnist_cnn_model import MNISTCNNModel
    ww, X, _ = cnn_ref.make_case(cnn_ref.MNIST, NV, SEED)
    model = MNISTCNNModel()
    with torch.no_grad():
        for p, layer in zip(model.parameters(), model.reshape(ww)):
            p.copy_(layer)
        logits = model(torch.from_numpy(X.reshape(NV, 1, 28, 28))).numpy()
    pred = np.argmax(logits, axis=1)
    lg, E = cnn_ref.forward(cnn_ref.MNIST, ww, X)
    flag = cnn_ref.near_ties(lg, E)
    assert np.array_equal(np.argmax(lg, axis=1)[~flag], pred[~flag])
    share = float(flag.mean())
    assert share <= 0.5, share
    np.savez(os.path.join(HERE, "cnn_mnist_logits.npz"), seed=SEED, logits=logits.astype(np.float32),
             pred=pred.astype(np.int32), share=share,
             max_abs_diff=float(np.abs(lg.astype(np.float64) - logits).max()))
    print("flagged share %.4f, max |logit - torch| %.3e" % (share, np.abs(lg - logits).max()))


if __name__ == "__main__":
    main(sys.argv[1])
