"""Polynomial commitments in bn256 G1 on the GPU (bk_commit_*):
the commitments of a peer's iteration in the reference's SECURE_AGG mode.

    CommitKey.from_points        PKG1 made resident (each point's MarshalBinary)
    CommitKey.create_commitment  createCommitment (kyber.go:533-562)
    CommitKey.verify_commitment  verifyCommitment (kyber.go:564-577)
    CommitKey.generate_miner_commitments
                                 generateMinerSecretShares' commitments
                                 (kyber.go:456-482, 172-202, 579-646)

A point is its 64 marshalled bytes; infinity is 64 zero bytes.  Every array is
a host numpy array; Engine.commit_*_ptr take device memory.
"""
import numpy as np

from .krum import Engine, default_engine
from .shares import POLY_SIZE, PRECISION

__all__ = ["CommitKey", "create_commitment", "verify_commitment", "generate_miner_commitments"]


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
