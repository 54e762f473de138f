"""Polynomial commitments in bn256 G1 on the GPU (bk_commit_*):
the commitments of a peer's iteration in the reference's SECURE_AGG mode.

    CommitKey.from_points        PKG1 made resident (each point's MarshalBinary)
    CommitKey.create_commitment  createCommitment (kyber.go:533-562)
    CommitKey.verify_commitment  verifyCommitment (kyber.go:564-577)
    CommitKey.generate_miner_commitments
                                 generateMinerSecretShares' commitments
                                 (kyber.go:456-482, 172-202, 579-646)
    PointStore                   the miner: the points of the clients' parts and
                                 their sums over the agreed node list
                                 (aggregateSecret, kyber.go:244-287), the twin
                                 of shares.ShareStore

A point is its 64 marshalled bytes; infinity is 64 zero bytes.  Every array is
a host numpy array; Engine.commit_*_ptr take device memory.
"""
import numpy as np

from .krum import Engine, default_engine
from .shares import POLY_SIZE, PRECISION

__all__ = ["CommitKey", "create_commitment", "verify_commitment", "generate_miner_commitments",
           "PointStore"]


class CommitKey:
    """The resident key of an engine: one per engine, replaced by the next
    from_points on it."""

    def __init__(self, engine, count):
        self.engine, self.count = engine, count

    @classmethod
    def from_points(cls, points, engine: Engine = None):
        eng = engine or default_engine()
        eng.commit_set_key(points)
        return cls(eng, eng.commit_key_count())

    def __len__(self):
        return self.count

    def create_commitment(self, update_int, first=0):
        """The 64 bytes of sum update_int[i] PK[first + i]."""
        return self.engine.commit_msm(np.asarray(update_int), first)

    def verify_commitment(self, update_int, committed, first=0):
        return self.engine.commit_verify(np.asarray(update_int), committed, first)

    def generate_miner_commitments(self, delta, precision=PRECISION, poly_size=POLY_SIZE,
                                   total_shares=20):
        """(commitment 64, chunk commitments chunks x 64, witnesses chunks x
        total_shares x 64) as uint8 arrays, of a float64 delta (quantised with
        `precision`) or of an int64 update taken as it is."""
        return self.engine.commit_generate(delta, precision, poly_size, total_shares)


def _key(key):
    if not isinstance(key, CommitKey):
        raise ValueError("key must be a CommitKey (CommitKey.from_points)")
    return key


def create_commitment(key, update_int, first=0):
    return _key(key).create_commitment(update_int, first)


def verify_commitment(key, update_int, committed, first=0):
    return _key(key).verify_commitment(update_int, committed, first)


def generate_miner_commitments(key, delta, precision=PRECISION, poly_size=POLY_SIZE,
                               total_shares=20):
    return _key(key).generate_miner_commitments(delta, precision, poly_size, total_shares)


class PointStore:
    """One miner's G1 points of an iteration, on the GPU, one part per client:
    the client's commitment, its chunk commitments and the miner's `held`
    witnesses of every chunk."""

    def __init__(self, chunks, held, n_cap, engine: Engine = None):
        self.engine = engine or default_engine()
        self.engine.commit_points_begin(chunks, held, n_cap)
        self._slot = {}

    def add_part(self, node_id, commit, chunk_pts, witness_pts):
        """The points client node_id sent; a client registers once.  A point that
        does not unmarshal refuses the part (ValueError) and takes no slot."""
        if node_id in self._slot:
            raise ValueError("node %r has already registered a part" % (node_id,))
        self._slot[node_id] = self.engine.commit_points_add(commit, chunk_pts, witness_pts)

    def __len__(self):
        return len(self._slot)

    def miner_points(self, node_list):
        """(commitment 64, chunk commitments chunks x 64, witnesses chunks x held
        x 64), uint8: the sums of the listed clients' points, what GetMinerPart's
        reply carries beside ShareStore.miner_part."""
        missing = [n for n in node_list if n not in self._slot]
        if missing:
            raise ValueError("no part from node(s) %r" % (missing,))
        return self.engine.commit_points_sum(
            np.array([self._slot[n] for n in node_list], dtype=np.int64))
