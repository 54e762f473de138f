"""The convergence check on libbk: the new model's error and attack rate.

checkConvergence (DistSys/honest.go:141-162) scores the model of every appended
block: testModel (honest.go:656-675, bound to train_error / getTestErr) and,
for the torch datasets, testAttackRate (honest.go:260-275, bound to
get17AttackRate).  ModelEvaluator keeps the sets those functions read resident
on the GPU (bk_eval_set_*) and scores a model in one launch (bk_eval):

    logistic  sum(sign(X . w) != y) / float(y.size)    ML/code/logistic_model_test.py:13-24
    softmax   1 - accuracy_score(argmax(model(x)), y)  ML/Pytorch/client.py:146-172

The arithmetic runs in libbk.so on the GPU; there is no CPU path.
"""
from typing import Optional

import numpy as np

from .krum import Engine, default_engine

__all__ = ["ModelEvaluator", "TRAIN", "TEST", "ATTACK"]

TRAIN, TEST, ATTACK = 0, 1, 2  # the evaluation-set slots of the engine's context


class ModelEvaluator:
    """train / test / attack: (X, y) pairs, any of them None.  n_classes None:
    the logistic model (X float64, labels as numbers, a model of d weights);
    otherwise the softmax model (X float32, integer labels, a model of
    n_classes * (d_in + 1) entries: W row-major, then b).

    One evaluator per engine at a time: the sets live in the engine's context
    (slots TRAIN, TEST, ATTACK)."""

    def __init__(self, train=None, test=None, attack=None, n_classes: Optional[int] = None,
                 engine: Optional[Engine] = None):
        given = [(slot, s) for slot, s in ((TRAIN, train), (TEST, test), (ATTACK, attack))
                 if s is not None]
        if not given:
            raise ValueError("an evaluator needs a train, test or attack set")
        if n_classes is not None and not 2 <= int(n_classes) <= 16:
            raise ValueError("n_classes must be in [2, 16]")
        cols = set()
        sets = []
        for slot, s in given:
            if len(s) != 2:
                raise ValueError("a set is an (X, y) pair")
            X = np.asarray(s[0])
            want = np.float64 if n_classes is None else np.float32
            if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
                raise ValueError("X must be a matrix, samples x features")
            X = np.ascontiguousarray(X, dtype=want)
            y = np.asarray(s[1])
            if y.shape != (X.shape[0],):
                raise ValueError("y must have one label per row of X")
            cols.add(X.shape[1])
            sets.append((slot, X, y))
        if len(cols) != 1:
            raise ValueError("the sets must have the same number of features")
        self.n_classes = None if n_classes is None else int(n_classes)
        self.d_in = cols.pop()
        self.d = self.d_in if n_classes is None else self.n_classes * (self.d_in + 1)
        self._engine = engine if engine is not None else default_engine(0)
        self._slots = []
        for slot, X, y in sets:
            if self.n_classes is None:
                self._engine.eval_set_logistic(slot, X, y)
            else:
                self._engine.eval_set_softmax(slot, X, y, self.n_classes)
            self._slots.append(slot)
        self.near_ties = {}  # slot -> the last evaluation's near-tie count (softmax)

    def _has(self, slot):
        return slot in self._slots

    def evaluate(self, ww, slots):
        """{slot: (err, wrong)} of the model on the slots named, one launch."""
        for s in slots:
            if not self._has(s):
                raise ValueError("the evaluator has no set in slot %d" % s)
        err, wrong, near = self._engine.eval(ww, list(slots))
        return self._record(slots, err, wrong, near)

    def _record(self, slots, err, wrong, near):
        for i, s in enumerate(slots):
            self.near_ties[s] = int(near[i])
        return {s: (float(err[i]), int(wrong[i])) for i, s in enumerate(slots)}

    def train_error(self, ww) -> float:
        return self.evaluate(ww, [TRAIN])[TRAIN][0]

    def test_error(self, ww) -> float:
        return self.evaluate(ww, [TEST])[TEST][0]

    def attack_rate(self, ww) -> float:
        return self.evaluate(ww, [ATTACK])[ATTACK][0]

    def convergence_slots(self):
        """The sets checkConvergence reads: the train set (the test set if there
        is no train set), and the attack set if there is one."""
        slots = [TRAIN if self._has(TRAIN) else TEST]
        if not self._has(slots[0]):
            raise ValueError("check_convergence needs a train or test set")
        if self._has(ATTACK):
            slots.append(ATTACK)
        return slots

    def _verdict(self, res, slots, threshold):
        err = res[slots[0]][0]
        rate = res[ATTACK][0] if ATTACK in slots else None
        return err < threshold, err, rate

    def check_convergence(self, ww, threshold):
        """honest.go:141-162: (converged, train_error, attack_rate or None);
        converged is train_error < threshold.  One launch for both sets."""
        slots = self.convergence_slots()
        return self._verdict(self.evaluate(ww, slots), slots, threshold)

    def finish_block(self, engine_call, threshold=None):
        """The evaluated form of a block's finish: engine_call(slots) is
        Engine.block_finish_eval bound to its other arguments.  Returns its
        block outputs and check_convergence's triple (threshold None: converged
        is None)."""
        slots = self.convergence_slots()
        out = engine_call(slots)
        err, wrong, near = out[-3:]
        res = self._record(slots, err, wrong, near)
        conv, e, rate = self._verdict(res, slots, np.inf if threshold is None else threshold)
        return out[:-3], (None if threshold is None else conv, e, rate)
