"""The gradient step on the GPU (bk_grad_*): what
computeUpdate -> oneGradientStep (DistSys/honest.go:165-200, 284-324) asks of
the peer's Python model every iteration, on the peer's shard held on the device.

    LogisticStepper   privateFun of ML/code/logistic_model.py:113-140 (funObj
                      :92-106): delta = -alpha * g [+ getNoise(iteration)]
    SoftmaxStepper    privateFun of ML/Pytorch/client_obj.py:73-77:
                      -Client.getGrad() (client.py:38-65: mean cross-entropy,
                      clip_grad_norm(., 100), W then b flattened)

Drawing the mini-batch (np.random.choice, the shuffled loader's first batch)
and pre-sampling the noise stay the caller's: both steppers take the batch's row
numbers and the iteration's noise vector.  There is no host fallback.
"""
import numpy as np

from .krum import Engine, default_engine

__all__ = ["LogisticStepper", "SoftmaxStepper"]


class _Stepper:
    loss = None   # the last step's loss (the reference's f / Client.loss)
    norm = None   # softmax: the last step's gradient norm before clipping

    def _result(self, delta, q, precision):
        return delta if precision is None else (delta, q)


class LogisticStepper(_Stepper):
    """One peer's logistic model: X nn x d float64 (bias column included, as
    utils.load_dataset returns it), y the nn labels (-1 / +1, or 0 / 1)."""

    def __init__(self, X, y, batch_size, alpha=1e-2, lammy=0.01, engine: Engine = None):
        X = np.asarray(X)
        if X.ndim != 2 or X.dtype != np.float64 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be a float64 matrix, nn x d")
        ya = np.asarray(y)
        if ya.shape != (X.shape[0],) or not (np.issubdtype(ya.dtype, np.integer)
                                             or np.issubdtype(ya.dtype, np.floating)):
            raise ValueError("y must have one numeric label per row of X")
        if not np.isfinite(ya.astype(np.float64)).all():
            raise ValueError("labels must be finite")
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            # the reference divides by this_batch_size: 0 raises ZeroDivisionError
            raise ValueError("batch_size=%d < 1" % self.batch_size)
        self.alpha, self.lammy = float(alpha), float(lammy)
        self.nn, self.d = X.shape
        self.engine = engine or default_engine()
        self.engine.grad_set_logistic(X, ya)

    def private_fun(self, ww, idx=None, noise=None, precision=None):
        """delta (and its int64 quantisation with a precision) for the model ww
        on the rows idx (None: every row, the reference's choice when
        batch_size >= nn)."""
        delta, q, self.loss = self.engine.grad_logistic(ww, idx, self.batch_size, self.alpha,
                                                        self.lammy, noise, precision)
        return self._result(delta, q, precision)


class SoftmaxStepper(_Stepper):
    """One peer's torch softmax model: X nn x d_in float32, y integer labels in
    [0, n_classes); the model is n_classes * (d_in + 1) float64 entries."""

    def __init__(self, X, y, n_classes, max_norm=100.0, engine: Engine = None):
        X = np.asarray(X)
        if X.ndim != 2 or X.dtype != np.float32 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be a float32 matrix, nn x d_in")
        self.n_classes = int(n_classes)
        if not 2 <= self.n_classes <= 16:
            raise ValueError("n_classes=%d outside [2, 16]" % self.n_classes)
        ya = np.asarray(y)
        if ya.shape != (X.shape[0],) or not np.issubdtype(ya.dtype, np.integer):
            raise ValueError("y must have one integer label per row of X")
        if ya.min() < 0 or ya.max() >= self.n_classes:
            raise ValueError("labels outside [0, %d)" % self.n_classes)
        self.max_norm = float(max_norm)
        if not (np.isfinite(self.max_norm) and self.max_norm > 0.0):
            raise ValueError("max_norm must be a positive finite number")
        self.nn, self.d_in = X.shape
        self.d = self.n_classes * (self.d_in + 1)
        self.engine = engine or default_engine()
        self.engine.grad_set_softmax(X, ya, self.n_classes)

    def private_fun(self, ww, idx=None, noise=None, precision=None):
        delta, q, self.loss, self.norm = self.engine.grad_softmax(ww, idx, self.max_norm, noise,
                                                                  precision)
        return self._result(delta, q, precision)
