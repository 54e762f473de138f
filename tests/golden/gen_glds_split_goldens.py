"""Record K1's bits before the glds split moved off the staggered waves.

    LIB=/path/to/the/parent/commit's/libbk.so python tests/golden/gen_glds_split_goldens.py

Run ONCE on an MI355X with the library built from the commit BEFORE the split
changed (which wave issues which global_load_lds, and where): the change keeps
every MFMA and its order, so the packed upper triangle, the selection, the
scores and the mean of a later library must equal these files bit for bit
(tests/test_gpu_gram_glds_split.py).  The inputs are rebuilt from integers
(`rows`), so the files hold only the results and the input's SHA-256.

A packed upper triangle above 512 KiB (n = 512: 1.18 MB) is stored as its
SHA-256 and every 16th element (equality of the digest is equality of the
bits; the sample says where a mismatch sits).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FULL_UPPER_BYTES = 512 * 1024
SAMPLE = 16

# name: (n, d, f, row dtype, f32 mode) -- each the smallest shape that reaches one path
CASES = {
    "glds_n512_d4112": (512, 4112, 153, "float64", "exact"),      # both group kinds, NB = 4 and 6, 257 k-blocks
    "glds_n130_d4100": (130, 4100, 39, "float64", "exact"),       # one lone super-block, run-time NB, ragged tail
    "glds_n320_d2064": (320, 2064, 96, "float64", "exact"),       # odd super-block count: quad + lone + pairs
    "glds_n512_d48": (512, 48, 153, "float64", "exact"),          # three k-blocks: the prologue fills the ring
    "glds_n512_d16": (512, 16, 153, "float64", "exact"),          # one k-block
    "glds_n512_d4112_f32": (512, 4112, 153, "float32", "exact"),  # widened fp32 rows, 32-column k-blocks
    "glds_n512_d4096_f32mfma": (512, 4096, 153, "float32", "mfma"),  # the unstaggered instance (even split)
}


def rows(name):
    """The case's input, from integers alone (the same bits on every numpy)."""
    n, d, f, dt, _ = CASES[name]
    rng = np.random.Generator(np.random.PCG64(sorted(CASES).index(name) + 2024))
    q = rng.integers(-(1 << 30), 1 << 30, size=(n, d), dtype=np.int64)
    mu = rng.integers(-(1 << 30), 1 << 30, size=d, dtype=np.int64)
    X = mu.astype(np.float64) * (0.01 * 2.0 ** -30) + q.astype(np.float64) * (1e-3 * 2.0 ** -30)
    X[: n // 3] += q[::-1][: n // 3].astype(np.float64) * (0.05 * 2.0 ** -30)  # the Byzantine third
    return np.ascontiguousarray(X.astype(dt))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(engine, name):
    """upper, sel, scores, mean of one case on `engine` (numpy arrays)."""
    import torch
    from biscotti_amd import _lib
    n, d, f, dt, mode = CASES[name]
    code = _lib.BK_F32 if dt == "float32" else _lib.BK_F64
    X = torch.from_numpy(rows(name)).cuda()
    U = torch.empty(int(_lib.lib().bk_upper_elems(n)), dtype=torch.float64, device="cuda")
    sel = torch.empty(n - f, dtype=torch.int64, device="cuda")
    sc = torch.empty(n, dtype=torch.float64, device="cuda")
    mean = torch.empty(d, dtype=torch.float64, device="cuda")
    engine.set_f32_mode(_lib.BK_F32_MFMA if mode == "mfma" else _lib.BK_F32_EXACT)
    try:
        engine.gram_upper_ptr(X.data_ptr(), code, n, d, d, U.data_ptr())
        engine.multikrum_device_ptr(X.data_ptr(), code, n, d, d, f, sel.data_ptr(), sc.data_ptr(),
                                    mean.data_ptr())
        engine.synchronize()
    finally:
        engine.set_f32_mode(_lib.BK_F32_EXACT)
    return U.cpu().numpy(), sel.cpu().numpy(), sc.cpu().numpy(), mean.cpu().numpy()


def record(name, U, sel, sc, mean):
    rec = {"input_sha256": np.array(digest(rows(name))), "sel": sel, "scores": sc, "mean": mean,
           "upper_sha256": np.array(digest(U))}
    if U.nbytes <= FULL_UPPER_BYTES:
        rec["upper"] = U
    else:
        rec["upper_sample"] = U[::SAMPLE].copy()
    return rec


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    from biscotti_amd import _lib
    if os.environ.get("LIB"):
        _lib.LIB_PATH = os.path.abspath(os.environ["LIB"])
    from biscotti_amd.krum import Engine
    out = os.environ.get("OUT", HERE)
    os.makedirs(out, exist_ok=True)
    e = Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    for name in CASES:
        rec = record(name, *run(e, name))
        path = os.path.join(out, name + ".npz")
        np.savez_compressed(path, **rec)
        print("%s: %d bytes, upper %s, library %s" % (name, os.path.getsize(path),
                                                     str(rec["upper_sha256"])[:16], _lib.LIB_PATH), flush=True)
    e.close()


if __name__ == "__main__":
    main()
