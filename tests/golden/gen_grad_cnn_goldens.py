"""Golden vectors for the one-layer CNN's gradient step (bk_grad_cnn, DESIGN.md
§5z), produced by the REFERENCE's own code on repo-owned inputs.  Run on the CPU:

    python tests/golden/gen_grad_cnn_goldens.py <reference>/ML/Pytorch

``Client.getGrad`` (client.py:38-65) on the reference's ``MNISTCNNModel`` after
``Client.updateModel``, driven as gen_grad_goldens.py drives the softmax model:
a one-batch loader, Client.__init__'s criterion and optimizer, clip_grad_norm
wrapped to record the norm it returns; the result negated as
client_obj.privateFun (:73-77) does.  The inputs are cnn_ref.make_case(MNIST,
nn, seed), the model times `wscale`; the tests rebuild them and check their
SHA-256.  The clipped case doubles wscale until torch's norm exceeds 100.

A condition on the inputs, asserted here (a seed that fails it is replaced,
the condition never relaxed): a forward hook on layer1[0] gives torch's own
pre-activations, and every (sample, feature) is > 0 in both torch's values and
grad_cnn_ref's, or <= 0 in both -- a ReLU that differs in sign moves a
conv-gradient entry by a whole term.

Saved per case (.npz): idx, delta (float32: what torch computed), loss, norm and
the inputs' hashes.  grad_cnn_cases.json keeps the parameters, the scale, the
gate (grad_cnn_ref.torch_gate) and the deviation of grad_cnn_ref from torch
measured here in units of the scale; no case may be above its gate.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import cnn_ref  # noqa: E402
import grad_cnn_ref as R  # noqa: E402
import gen_grad_goldens as GG  # noqa: E402
import gen_roni_softmax_goldens as RS  # noqa: E402
import gen_eval_goldens as E  # noqa: E402

CASES = {
    "grad_cnn_mnist": dict(seed=3001, nn=24, count=10, wscale=1.0),
    "grad_cnn_clip": dict(seed=3002, nn=24, count=10, wscale=None),
}


def run_reference(client, model_cls, ww, Xb, yb, recorded):
    import torch
    c = client.Client.__new__(client.Client)
    c.model = model_cls()
    c.criterion = client.nn.CrossEntropyLoss()
    c.optimizer = client.optim.SGD(c.model.parameters(), lr=0.001, momentum=0.75, weight_decay=0.001)
    c.loss = 0.0
    c.trainloader = E.loader([(np.ascontiguousarray(Xb.reshape(len(Xb), 1, 28, 28)), yb)])
    c.updateModel(np.array(ww))
    pre = []
    c.model.layer1[0].register_forward_hook(lambda mod, i, o: pre.append(o.detach().numpy().copy()))
    del recorded[:]
    with torch.enable_grad():
        delta = (-1) * np.asarray(c.getGrad(), dtype=np.float64)
    return delta, float(c.getLoss()), recorded[-1], pre[-1]


def main(ref_dir):
    RS.REF = ref_dir
    client, _ = RS.load_reference()
    sys.path.insert(0, ref_dir)
    from mnist_cnn_model import MNISTCNNModel
    recorded = []
    clip = client.nn.utils.clip_grad_norm

    def recording_clip(*args, **kw):
        v = clip(*args, **kw)
        recorded.append(float(v))
        return v

    client.nn.utils.clip_grad_norm = recording_clip
    manifest = {}
    for name, p in CASES.items():
        ww0, X, y = cnn_ref.make_case(cnn_ref.MNIST, p["nn"], p["seed"])
        idx = GG.draw_idx(p["seed"], p["nn"], p["count"])
        wscale = p["wscale"] or 1.0
        while True:
            ww = ww0 * wscale
            delta, loss, norm, pre = run_reference(client, MNISTCNNModel, ww, X[idx], y[idx], recorded)
            if p["wscale"] is not None or norm > 100.0:
                break
            wscale *= 2.0
        _, mypre, _ = R.activations(cnn_ref.MNIST, ww, X[idx].astype(np.float64))
        assert np.array_equal(pre > 0, mypre > 0), (name, int(((pre > 0) != (mypre > 0)).sum()))
        mine, myloss, mynorm = R.step(cnn_ref.MNIST, X, y, ww, idx)
        scale = R.scale(cnn_ref.MNIST, X, ww, idx)
        gate = R.torch_gate(cnn_ref.MNIST, p["count"])
        dev = float(np.max(np.abs(mine - delta)) / scale)
        assert np.isfinite(delta).all() and dev <= gate, (name, dev, gate)
        np.savez(os.path.join(HERE, name + ".npz"), idx=idx, delta=delta.astype(np.float32),
                 loss=np.array(loss), norm=np.array(norm), X_sha256=GG.sha(X), y_sha256=GG.sha(y),
                 ww_sha256=GG.sha(ww))
        manifest[name] = dict(p, wscale=wscale, scale=scale, norm=norm, gate=gate, ref_deviation=dev,
                              norm_deviation=abs(mynorm - norm) / norm,
                              loss_deviation=abs(myloss - loss) / max(abs(loss), 1.0))
        print(name, "wscale", wscale, "norm", norm, "deviation", dev, "gate", gate, flush=True)
    with open(os.path.join(HERE, "grad_cnn_cases.json"), "w") as fp:
        json.dump(manifest, fp, indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1])
