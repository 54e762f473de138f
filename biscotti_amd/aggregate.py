"""Host-side mirror of the steps either side of the Multi-Krum verifier
(SURVEY.md §8(f) rows 2 and 3), on libbk.

  create_block(global_w, block_updates, stake_map)
        Honest.createBlock, DistSys/honest.go:346-381: GlobalW += Delta of
        every accepted update, in blockUpdates order (bk_aggregate), and the
        +-STAKE_UNIT stake bookkeeping (honest.go:46, :364-369; host logic).
  quantized_sum(deltas, idx, precision)
        updateFloatToInt (DistSys/kyber.go:698-710) of each accepted update,
        summed as the miners' share aggregation does (honest.go:401-409,
        442-502), and updateIntToFloat (kyber.go:745-757)
        (bk_quantized_sum_device).
  apply_noise(delta, noise)
        requestNoiseFromNoisers' average (DistSys/main.go:1606-1653) added
        to Delta (main.go:1524-1537), batched over updates
        (bk_noise_apply_device).

The arithmetic runs in libbk.so on the GPU (torch only moves buffers); there
is no CPU path.
"""
from typing import Dict, List, Optional, Sequence

import numpy as np

from .krum import Engine, Update, _dtype_code, default_engine

__all__ = ["STAKE_UNIT", "PRECISION", "create_block", "quantized_sum", "apply_noise",
           "BlockCollector"]

STAKE_UNIT = 5   # DistSys/honest.go:46
PRECISION = 4    # DistSys/main.go:45


def _engine(engine: Optional[Engine]) -> Engine:
    return engine if engine is not None else default_engine(0)


def create_block(global_w: np.ndarray, block_updates: Sequence[Update],
                 stake_map: Dict[int, int], engine: Optional[Engine] = None) -> np.ndarray:
    """honest.go:346-381 minus the chain append: returns the updated gradient
    (a new array, like mat.Row into updatedGradient) and updates stake_map in
    place.  Accepted updates are added in blockUpdates order."""
    out = np.array(global_w, dtype=np.float64, copy=True)
    d = out.shape[0]
    accepted: List[int] = []
    for i, u in enumerate(block_updates):
        their = stake_map.get(u.SourceID, 0)
        if u.Accepted:
            accepted.append(i)
            stake_map[u.SourceID] = their + STAKE_UNIT
        else:
            stake_map[u.SourceID] = their - STAKE_UNIT
    if not accepted:
        return out
    X = np.empty((len(block_updates), d), dtype=np.float64)
    for i, u in enumerate(block_updates):
        if u.Accepted:
            delta = np.asarray(u.Delta, dtype=np.float64)
            if delta.shape != (d,):
                raise ValueError("update %d: Delta has %s entries, gradient has %d"
                                 % (i, delta.shape, d))
            X[i] = delta
        else:
            X[i] = 0.0  # never read
    _engine(engine).aggregate(X, np.asarray(accepted, dtype=np.int64), out)
    return out


class BlockCollector:
    """The miner's side of a block, with every add done as its update arrives
    (bk_block_*): addBlockUpdate (DistSys/honest.go:330-334) uploads Delta and
    adds it to the running gradient at once, createBlock (honest.go:346-388)
    reads the gradient back and does the stake bookkeeping.  The result equals
    create_block(global_w, updates, stake_map) bitwise: the adds are the same
    sequential fp64 adds in arrival order.

    precision: None, or the PRECISION of the secure path, whose running int64
    sum quantized_sum() returns.  One collector per engine at a time (the
    engine's context holds one block)."""

    def __init__(self, global_w, precision: Optional[int] = None,
                 engine: Optional[Engine] = None, dtype=np.float64):
        self._engine = _engine(engine)
        self._g0 = np.array(global_w, dtype=np.float64, copy=True)
        if self._g0.ndim != 1 or self._g0.shape[0] < 1:
            raise ValueError("global_w must be a vector")
        self._precision = precision
        self._dtype = np.dtype(dtype)
        self.flush()

    def flush(self):
        """Restart the block from the gradient it was made with."""
        self._updates: List[Update] = []
        self._result = None   # the fused last add's gradient, until another add
        self._qsum = None
        self._engine.block_begin(self._g0, self._precision, self._dtype)

    def add_update(self, update: Update, last: bool = False) -> int:
        """addBlockUpdate: append the update and add its Delta on the device if
        it is accepted (a rejected update's Delta is never read).  last=True is
        the NUM_SAMPLES / 2-th arrival: the add and the finish in one engine
        call.  Returns the number of updates in the block."""
        d = self._g0.shape[0]
        row = None
        if update.Accepted:
            row = np.asarray(update.Delta, dtype=self._dtype)
            if row.shape != (d,):
                raise ValueError("update %d: Delta has %s entries, gradient has %d"
                                 % (len(self._updates), row.shape, d))
        elif last:
            row = np.zeros(d, dtype=self._dtype)  # the entry wants a row; it is never read
        want_q = self._precision is not None
        if last:
            out = self._engine.block_add_finish(row, bool(update.Accepted), want_qsum=want_q)
            self._result = out[1]
            self._qsum = (out[2], out[3]) if want_q else None
        else:
            self._engine.block_add([row], [1 if update.Accepted else 0])
            self._result = self._qsum = None
        self._updates.append(update)
        return len(self._updates)

    def _finish(self):
        if self._result is None:
            want_q = self._precision is not None
            out = self._engine.block_finish(want_qsum=want_q)
            self._result = out[0] if want_q else out
            self._qsum = (out[1], out[2]) if want_q else None
        return self._result

    def create_block(self, stake_map: Dict[int, int], evaluator=None, threshold=None):
        """createBlock over the updates added so far (the deadline path may call
        it with fewer than expected): the updated gradient, a new array, and the
        +-STAKE_UNIT bookkeeping on stake_map.  The block is not consumed.

        evaluator (an evaluate.ModelEvaluator on this collector's engine): the
        new gradient is also scored where it is, on the device
        (bk_block_finish_eval), and the return value is (gradient, (converged,
        train_error, attack_rate or None)) -- checkConvergence's answer
        (honest.go:141-162; converged is None without a threshold)."""
        for u in self._updates:
            their = stake_map.get(u.SourceID, 0)
            stake_map[u.SourceID] = their + (STAKE_UNIT if u.Accepted else -STAKE_UNIT)
        if evaluator is None:
            return self._finish().copy()
        want_q = self._precision is not None
        out, verdict = evaluator.finish_block(
            lambda slots: self._engine.block_finish_eval(slots, want_qsum=want_q), threshold)
        self._result = out[0]
        self._qsum = (out[1], out[2]) if want_q else None
        return self._result.copy(), verdict

    def quantized_sum(self):
        """(int64 sum, float64 sum) of the accepted updates so far, as
        quantized_sum() over them gives."""
        if self._precision is None:
            raise ValueError("the collector was made without a precision")
        self._finish()
        return self._qsum[0].copy(), self._qsum[1].copy()


def quantized_sum(deltas, idx, precision: int = PRECISION, engine: Optional[Engine] = None):
    """(int64 sum, float64 sum) over rows idx of deltas (n x d), each row
    quantised as int64(x * 10^precision) (Go amd64 truncation)."""
    import torch
    eng = _engine(engine)
    X = np.ascontiguousarray(deltas)
    if X.dtype not in (np.float64, np.float32):
        X = X.astype(np.float64)
    n, d = X.shape
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("idx out of range [0, %d)" % n)
    dev = torch.device("cuda", eng.device)
    tX = torch.from_numpy(X).to(dev)
    tI = torch.from_numpy(idx).to(dev)
    s = torch.empty(d, dtype=torch.int64, device=dev)
    sf = torch.empty(d, dtype=torch.float64, device=dev)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.quantized_sum_ptr(tX.data_ptr(), _dtype_code(X.dtype), n, d, d, tI.data_ptr(), len(idx),
                          precision, s.data_ptr(), sf.data_ptr())
    torch.cuda.synchronize(dev)
    return s.cpu().numpy(), sf.cpu().numpy()


def apply_noise(delta, noise, engine: Optional[Engine] = None) -> np.ndarray:
    """NoisedDelta for a batch: delta (n x d) or (d,), noise (n x k x d) or
    (k x d) -- noise vectors in arrival order."""
    import torch
    eng = _engine(engine)
    D = np.ascontiguousarray(delta, dtype=np.float64)
    N = np.ascontiguousarray(noise, dtype=np.float64)
    single = D.ndim == 1
    if single:
        D, N = D[None], N[None]
    n, d = D.shape
    if N.ndim != 3 or N.shape[0] != n or N.shape[2] != d:
        raise ValueError("noise must be (n, k, d) matching delta (n, d)")
    k = N.shape[1]
    dev = torch.device("cuda", eng.device)
    tD = torch.from_numpy(D).to(dev)
    tN = torch.from_numpy(N.reshape(n * k, d) if k else np.zeros((1, d))).to(dev)
    out = torch.empty_like(tD)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.noise_apply_ptr(tD.data_ptr(), n, d, d, tN.data_ptr(), k, d, out.data_ptr(), d)
    torch.cuda.synchronize(dev)
    o = out.cpu().numpy()
    return o[0] if single else o
