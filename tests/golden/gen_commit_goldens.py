"""Writes tests/golden/commit_d2561.npz from the pure-Python oracle
(tests/commit_ref.py): d = 2,561 is 257 chunks of 10 coefficients, the last of
one.  The whole commitment, every chunk commitment and the witnesses of chunks
0, 127, 255 and 256, over the key PK[i] = 2^i G.

    python tests/golden/gen_commit_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import commit_ref as C  # noqa: E402
import shares_ref as S  # noqa: E402

D, P, T, PREC = 2561, 10, 20, 4
CHUNKS = (0, 127, 255, 256)


def main():
    delta = np.random.default_rng(2561).normal(0.0, 0.1, size=D)
    q = S.quantize(delta, PREC)
    key = C.key_powers(D)
    whole, cc, ww = C.generate(q, key, P, T, chunks=set(CHUNKS))
    np.savez_compressed(os.path.join(HERE, "commit_d2561.npz"), delta=delta,
                        q=np.array(q, dtype=np.int64), commit=C.as_array([whole])[0],
                        chunk=C.as_array(cc), witness_chunks=np.array(CHUNKS, dtype=np.int64),
                        witness=np.stack([C.as_array(ww[c]) for c in CHUNKS]),
                        params=np.array([D, P, T, PREC], dtype=np.int64))


if __name__ == "__main__":
    main()
