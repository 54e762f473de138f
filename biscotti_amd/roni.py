"""Host-side mirror of Biscotti's RONI verifier, on libbk.

  roni(ww, delta)                 ML/code/logistic_validator.py:22-33 (the
                                  validation set is the module's, set once
                                  with set_validation -- the module body loads
                                  it at import, :6-7)
  RONIValidator                   Honest.verifyUpdate, DistSys/honest.go:598-629
    .verify_update(update)        Peer.VerifyUpdateRONI, DistSys/main.go:191-233:
                                  accept iff PRIV_PROB > 0 or score <= 0.02
    .scores(ww, deltas)           the batched form (one launch for n updates)
    .begin_round(ww)              the deployed form: the iteration's model held
    .score_round(deltas)          on the GPU with its evaluation done, each
                                  update scored on its own (bk_roni_round_*);
                                  verify_update(..., round=True) drives it

Everything runs through libbk.so on the GPU (bk_roni_set_validation / bk_roni);
there is no CPU path.
"""
from typing import Optional, Sequence

import ctypes

import numpy as np

from ._lib import BK_HOST, check, lib
from .krum import Engine, Update, default_engine

__all__ = ["RONI_THRESHOLD", "RONIValidator", "SoftmaxRONIValidator", "set_validation", "roni"]

RONI_THRESHOLD = 0.02  # main.go:213


class RONIValidator:
    """One validation set resident on one GPU (bk_roni_set_validation)."""

    def __init__(self, Xvalid, yvalid, engine: Optional[Engine] = None, priv_prob: float = 0.0):
        self._engine = engine if engine is not None else default_engine(0)
        X = np.ascontiguousarray(Xvalid, dtype=np.float64)
        y = np.ascontiguousarray(yvalid, dtype=np.float64)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError("Xvalid must be (nv, d) and yvalid (nv,)")
        self.nv, self.d = X.shape
        self.priv_prob = priv_prob  # PRIV_PROB > 0 accepts every update (main.go:205-211)
        check(lib().bk_roni_set_validation(self._engine.ctx, X.ctypes.data, self.nv, self.d,
                                           self.d, y.ctypes.data))

    def scores(self, ww, deltas) -> np.ndarray:
        ww = np.ascontiguousarray(ww, dtype=np.float64)
        D = np.ascontiguousarray(np.atleast_2d(deltas), dtype=np.float64)
        if ww.shape != (self.d,) or D.shape[1] != self.d:
            raise ValueError("ww must be (d,) and deltas (n, d) with d = %d" % self.d)
        out = np.empty(D.shape[0], dtype=np.float64)
        check(lib().bk_roni(self._engine.ctx, ww.ctypes.data, D.ctypes.data, D.shape[0], self.d,
                            self.d, out.ctypes.data))
        return out

    def roni(self, ww, delta) -> float:
        return float(self.scores(ww, np.asarray(delta)[None])[0])

    # ---- rounds: bc.getLatestGradient() is the same model for every update
    #      of an iteration (honest.go:598-629), so it is evaluated once ------
    _round_ww = None   # the held model's host copy
    rounds_begun = 0   # begin_round calls (verify_update(round=True): one per distinct model)
    last_score = None  # the score behind the last verify_update verdict

    def _begin(self, ww):
        check(lib().bk_roni_round_begin(self._engine.ctx, ww.ctypes.data, self.d, BK_HOST))

    def _score(self, rows, out):
        check(lib().bk_roni_round_score(self._engine.ctx, rows, len(rows), BK_HOST,
                                        out.ctypes.data))

    def begin_round(self, ww):
        """Hold ww on the GPU with its evaluation done (bk_roni*_round_begin)."""
        ww = np.array(ww, dtype=np.float64, order="C")  # the validator's own copy
        if ww.shape != (self.d,):
            raise ValueError("ww must be (d,) with d = %d" % self.d)
        self._round_ww = None
        self._begin(ww)
        self._round_ww = ww
        self.rounds_begun += 1

    def score_round(self, deltas) -> np.ndarray:
        """Scores of separately allocated updates against the held model,
        bitwise scores(ww, deltas)'s (bk_roni*_round_score)."""
        if self._round_ww is None:
            raise ValueError("no round: call begin_round(ww) first")
        rows = [np.ascontiguousarray(r, dtype=np.float64) for r in deltas]
        if not rows or any(r.shape != (self.d,) for r in rows):
            raise ValueError("deltas must be a non-empty sequence of (d,) rows with d = %d" % self.d)
        out = np.empty(len(rows), dtype=np.float64)
        self._score((ctypes.c_void_p * len(rows))(*[r.ctypes.data for r in rows]), out)
        return out

    def _round_score_one(self, latest_gradient, delta) -> float:
        held = self._round_ww
        if held is None or not (latest_gradient is held or
                                np.array_equal(held, latest_gradient, equal_nan=True)):
            self.begin_round(latest_gradient)
        return float(self.score_round([delta])[0])

    def verify_update(self, update: Update, latest_gradient, round: bool = False) -> bool:
        """True = accept (sign), False = reject (updateError).  round=True
        begins a round when latest_gradient differs from the held model, then
        scores the one update against it: the same score, without evaluating
        the model again."""
        if round:
            score = self._round_score_one(latest_gradient, update.NoisedDelta)
        else:
            score = self.roni(latest_gradient, update.NoisedDelta)
        self.last_score = score
        if self.priv_prob > 0:
            return True
        return not (score > RONI_THRESHOLD)

    def verify_updates(self, updates: Sequence[Update], latest_gradient) -> np.ndarray:
        """The batched form: one launch scores every update."""
        sc = self.scores(latest_gradient, np.stack([u.NoisedDelta for u in updates]))
        if self.priv_prob > 0:
            return np.ones(len(updates), dtype=bool)
        return ~(sc > RONI_THRESHOLD)


class SoftmaxRONIValidator(RONIValidator):
    """The torch-path verifier (ML/Pytorch/client_obj.py:100-112: the mnist /
    lfw softmax models): err = 1 - accuracy of argmax(x W^T + b)
    (client.py:136-144), the flat weights [W (C x d_in), b (C)] rounded to fp32
    as SoftmaxModel.reshape does.  The client's training shard is resident on
    one GPU (bk_roni_softmax_set_validation).

    Which samples: getTrainErr walks the SHUFFLED trainloader (client.py:20)
    and returns the error of its LAST mini-batch, so `original` and `after`
    are each measured on a fresh random last batch of batch_size samples (10
    in Biscotti, DistSys/honest.go:47).  This mirror draws those batches as the
    DataLoader does -- a permutation per pass, the last batch its tail of
    nv % batch_size (or batch_size) samples -- from its own seeded generator,
    and scores them with bk_roni_softmax_batches.  batch_size=None (or >= nv)
    scores every evaluation over the whole set (bk_roni_softmax).

    After each call, last_near_ties holds the per-evaluation near-tie counts
    (bk.h: where torch's fp32 argmax may differ from this one) and last_idx
    the (n, 2, nb) sample indices it scored (None for whole-set scores): the
    reference's scores are random draws (client.py:136-144), so a decision is
    reproduced by passing last_idx back as idx, or by a fixed seed.  A
    validator built with seed=None draws from fresh OS entropy each run.

    Rounds: with batch_size=None, begin_round / score_round /
    verify_update(round=True) score over the whole set.  round_batches=True
    (opt-in) gives a mini-batch validator rounds too: the model is held once
    per iteration and each update is scored on its own two freshly drawn last
    batches (bk_roni_softmax_round_score_batches), bitwise what scores() of a
    same-seed validator returns."""

    def __init__(self, Xvalid, yvalid, n_classes, engine: Optional[Engine] = None,
                 priv_prob: float = 0.0, batch_size: Optional[int] = 10, seed=None,
                 round_batches: bool = False):
        self._engine = engine if engine is not None else default_engine(0)
        self.round_batches = bool(round_batches)
        X = np.ascontiguousarray(Xvalid, dtype=np.float32)
        y = np.ascontiguousarray(yvalid, dtype=np.int32)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError("Xvalid must be (nv, d_in) and yvalid (nv,)")
        self.nv, self.d_in = X.shape
        self.n_classes = int(n_classes)
        self.d = self.n_classes * (self.d_in + 1)
        self.priv_prob = priv_prob
        self.batch_size = None if batch_size is None or batch_size >= self.nv else int(batch_size)
        if self.batch_size is not None and self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self._rng = np.random.default_rng(seed)
        self.last_near_ties = None
        self.last_idx = None
        check(lib().bk_roni_softmax_set_validation(self._engine.ctx, X.ctypes.data, self.nv,
                                                   self.d_in, self.d_in, y.ctypes.data,
                                                   self.n_classes))

    def _begin(self, ww):
        check(lib().bk_roni_softmax_round_begin(self._engine.ctx, ww.ctypes.data, BK_HOST))

    def _score(self, rows, out):
        nt = np.empty(len(rows) + 1, dtype=np.int32)
        check(lib().bk_roni_softmax_round_score(self._engine.ctx, rows, len(rows), BK_HOST,
                                                out.ctypes.data, nt.ctypes.data))
        self.last_near_ties = nt
        self.last_idx = None

    def _mini_batch_rounds(self) -> bool:
        return self.round_batches and self.batch_size is not None

    def begin_round(self, ww):
        if self.batch_size is not None and not self.round_batches:
            raise ValueError("rounds score over the whole set: build the validator with "
                             "batch_size=None, or with round_batches=True for rounds that "
                             "score each update on its own two last mini-batches")
        super().begin_round(ww)

    def score_round(self, deltas, idx=None) -> np.ndarray:
        """Whole-set rounds: RONIValidator.score_round.  With round_batches=True
        and a mini-batch batch_size: each update's two last batches are drawn as
        scores() draws them (original, then after; or taken from idx, (n, 2,
        nb)), and scored against the held model
        (bk_roni_softmax_round_score_batches): bitwise scores(ww, deltas, idx)."""
        if not self._mini_batch_rounds():
            if idx is not None:
                raise ValueError("idx needs round_batches=True and a mini-batch batch_size")
            return super().score_round(deltas)
        if self._round_ww is None:
            raise ValueError("no round: call begin_round(ww) first")
        rows = [np.ascontiguousarray(r, dtype=np.float64) for r in deltas]
        n = len(rows)
        if not rows or any(r.shape != (self.d,) for r in rows):
            raise ValueError("deltas must be a non-empty sequence of (d,) rows with d = %d" % self.d)
        idx = self.draw_batches(n) if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        if idx.ndim != 3 or idx.shape[:2] != (n, 2) or idx.shape[2] < 1:
            raise ValueError("idx must be (n, 2, nb)")
        out = np.empty(n, dtype=np.float64)
        nt = np.empty((n, 2), dtype=np.int32)
        table = (ctypes.c_void_p * n)(*[r.ctypes.data for r in rows])
        check(lib().bk_roni_softmax_round_score_batches(self._engine.ctx, table, n, BK_HOST,
                                                        idx.ctypes.data, idx.shape[2],
                                                        out.ctypes.data, nt.ctypes.data))
        self.last_idx = idx
        self.last_near_ties = nt
        return out

    def verify_update(self, update: Update, latest_gradient, round: bool = False) -> bool:
        if round and self.batch_size is not None and not self.round_batches:
            raise ValueError("round=True needs batch_size=None or round_batches=True")
        return super().verify_update(update, latest_gradient, round)

    def last_batch(self) -> np.ndarray:
        """One shuffled pass's last mini-batch (DataLoader(shuffle=True))."""
        perm = self._rng.permutation(self.nv)
        nb = self.nv % self.batch_size or self.batch_size
        return perm[self.nv - nb:]

    def draw_batches(self, n) -> np.ndarray:
        """(n, 2, nb) indices: per update, the batch `original` then the batch
        `after` is scored on, in the reference's call order."""
        return np.array([[self.last_batch(), self.last_batch()] for _ in range(n)], dtype=np.int64)

    def scores(self, ww, deltas, idx=None) -> np.ndarray:
        ww = np.ascontiguousarray(ww, dtype=np.float64)
        D = np.ascontiguousarray(np.atleast_2d(deltas), dtype=np.float64)
        if ww.shape != (self.d,) or D.shape[1] != self.d:
            raise ValueError("ww must be (d,) and deltas (n, d) with d = %d" % self.d)
        n = D.shape[0]
        out = np.empty(n, dtype=np.float64)
        if idx is None and self.batch_size is None:
            nt = np.empty(n + 1, dtype=np.int32)
            check(lib().bk_roni_softmax(self._engine.ctx, ww.ctypes.data, D.ctypes.data, n,
                                        self.d, out.ctypes.data, nt.ctypes.data))
            self.last_near_ties = nt
            self.last_idx = None
            return out
        idx = self.draw_batches(n) if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        self.last_idx = idx
        if idx.ndim != 3 or idx.shape[:2] != (n, 2):
            raise ValueError("idx must be (n, 2, nb)")
        nt = np.empty((n, 2), dtype=np.int32)
        check(lib().bk_roni_softmax_batches(self._engine.ctx, ww.ctypes.data, D.ctypes.data, n,
                                            self.d, idx.ctypes.data, idx.shape[2],
                                            out.ctypes.data, nt.ctypes.data))
        self.last_near_ties = nt
        return out


_validator: Optional[RONIValidator] = None


def set_validation(Xvalid, yvalid, engine: Optional[Engine] = None):
    """The module-level validation set (logistic_validator.py:6-7)."""
    global _validator
    _validator = RONIValidator(Xvalid, yvalid, engine)
    return _validator


def roni(ww, delta) -> float:
    """logistic_validator.py:22-33 against the set given to set_validation."""
    if _validator is None:
        raise RuntimeError("call set_validation(Xvalid, yvalid) first (the module loads it)")
    return _validator.roni(ww, delta)
