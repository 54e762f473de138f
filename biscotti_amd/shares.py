"""Secure aggregation on the GPU (bk_shares_*): the share
arithmetic of the reference's SECURE_AGG mode (DistSys/main.go:151).

    generate_miner_shares   the client: generateMinerSecretShares (kyber.go:456-482)
    ShareStore              the miner: Peer.RegisterSecret / addSecretShare
                            (main.go:256-286, honest.go:338-342) and the reply to
                            GetMinerPart (main.go:459-485, aggregateSecret
                            kyber.go:244-287)
    recover_block           the leader: recoverAggregateUpdates and the model
                            update of createBlockSecAgg (honest.go:391-502)

The bn256 commitments and witnesses are not computed here.  Every array is a
host numpy array; Engine.shares_*_ptr take device memory.
"""
import numpy as np

from .krum import Engine, default_engine

__all__ = ["PRECISION", "POLY_SIZE", "X0", "shares_per_miner", "miner_nodes",
           "generate_miner_shares", "ShareStore", "recover_block"]

PRECISION = 4    # DistSys/main.go:45
POLY_SIZE = 10   # DistSys/main.go:46
X0 = 10          # share s sits at x = s - 10 (pointToHashVal, kyber.go:677-695)


def shares_per_miner(total_shares, num_miners):
    """extractMinerSecret's sharesPerMiner (kyber.go:217); the reference's
    slices need num_miners to divide total_shares."""
    total_shares, num_miners = int(total_shares), int(num_miners)
    if num_miners < 1 or total_shares % num_miners:
        raise ValueError("num_miners=%d must divide total_shares=%d" % (num_miners, total_shares))
    return total_shares // num_miners


def miner_nodes(miner, held):
    """The nodes x of miner `miner`'s shares [held m, held (m + 1))."""
    return np.arange(held * miner, held * (miner + 1), dtype=np.int64) - X0


def generate_miner_shares(delta, num_miners, precision=PRECISION, poly_size=POLY_SIZE,
                          total_shares=20, engine: Engine = None):
    """The per-miner parts of one client's delta (float64 vector): a list of
    num_miners int64 arrays, chunks x held, [chunk][share]."""
    held = shares_per_miner(total_shares, num_miners)
    eng = engine or default_engine()
    y = eng.shares_generate(np.asarray(delta), precision, poly_size, total_shares)
    return [np.ascontiguousarray(y[:, held * m:held * (m + 1)]) for m in range(num_miners)]


class ShareStore:
    """One miner's parts of an iteration, on the GPU, one per client."""

    def __init__(self, d, held, n_cap, poly_size=POLY_SIZE, engine: Engine = None):
        self.engine = engine or default_engine()
        self.engine.shares_begin(d, poly_size, held, n_cap)
        self._slot = {}

    def add_part(self, node_id, part):
        """The part client node_id sent (addSecretShare); a client registers once."""
        if node_id in self._slot:
            raise ValueError("node %r has already registered a part" % (node_id,))
        self._slot[node_id] = self.engine.shares_add(part)

    def __len__(self):
        return len(self._slot)

    def miner_part(self, node_list):
        """The sum of the listed clients' parts (GetMinerPart's reply); it also
        stays on the device as the engine's own aggregate, which recover_block
        takes as a None part."""
        missing = [n for n in node_list if n not in self._slot]
        if missing:
            raise ValueError("no part from node(s) %r" % (missing,))
        return self.engine.shares_sum(np.array([self._slot[n] for n in node_list], dtype=np.int64))


def recover_block(global_w, parts, xs, precision=PRECISION, poly_size=POLY_SIZE,
                  engine: Engine = None):
    """(new model, aggregate delta, bad chunks): the miners' summed parts (a
    sequence of chunks x held_i int64 arrays, None for the engine's own
    aggregate) at the nodes xs, recovered exactly and added to global_w."""
    eng = engine or default_engine()
    g, _, delta, bad = eng.shares_recover(global_w, parts, xs, precision, poly_size,
                                          want_coef=False)
    return g, delta, bad
