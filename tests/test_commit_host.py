"""bk_bn256.h on the host: tools/commit_host.cpp, a stand-alone program, is
built once plainly and once with the address and undefined-behaviour sanitizers
and run directly on a file of commands; every result line must equal the
oracle's (tests/commit_ref.py).  Nothing is loaded into Python.  No GPU."""
import os
import random
import shutil
import subprocess

import pytest

import commit_ref as C
import shares_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "commit_host.cpp")
INC = os.path.join(REPO, "biscotti_amd", "csrc")

EDGE = (list(range(-33, 34)) + [(1 << 63) - 1, S.INT64_MIN, 1 << 32, -(1 << 32), (1 << 60) + 1,
                                -((1 << 60) + 1)])


def _cxx():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(rocm), "no C++ compiler"
    return rocm


def _fx(v):
    return "%064x" % v


def _cases():
    """(command line, expected output line)."""
    rng = random.Random(256)
    p = C.P
    out = []
    vals = [0, 1, 2, p - 1, p - 2, (1 << 255), (1 << 256) % p, p >> 1] + \
           [rng.randrange(p) for _ in range(24)]
    for a in vals:
        for b in (vals[:8] + [rng.randrange(p) for _ in range(3)]):
            out.append(("fmul %s %s" % (_fx(a), _fx(b)), _fx(a * b % p)))
            out.append(("fadd %s %s" % (_fx(a), _fx(b)), _fx((a + b) % p)))
            out.append(("fsub %s %s" % (_fx(a), _fx(b)), _fx((a - b) % p)))
    for a in vals[:8] + vals[-6:]:
        out.append(("finv %s" % _fx(a), _fx(pow(a, p - 2, p))))
    pts = [C.G, C.INF, C.neg(C.G), C.double(C.G)] + [C.mul(C.G, rng.randrange(1, C.N))
                                                     for _ in range(5)]
    for a in pts:
        ha = C.marshal(a).hex()
        out.append(("rt " + ha, ha))
        out.append(("pdbl " + ha, C.marshal(C.double(a)).hex()))
        for b in pts:
            out.append(("padd %s %s" % (ha, C.marshal(b).hex()), C.marshal(C.add(a, b)).hex()))
        out.append(("padd %s %s" % (ha, C.marshal(C.neg(a)).hex()), C.ZERO64.hex()))
    pt = pts[4]
    hp = C.marshal(pt).hex()
    for v in EDGE:
        # the literal multiplication for a few, the fast one (checked against it
        # in test_commit_ref.py) for the rest
        times = C.mul if v in (-33, -1, 33, S.INT64_MIN, (1 << 63) - 1) else C.mul_fast
        out.append(("smul %d %s" % (v, hp), C.marshal(times(pt, v)).hex()))
    out.append(("smul 5 " + C.ZERO64.hex(), C.ZERO64.hex()))
    # sums: the doubling inside an addition, infinity in mid-sum, an infinity key
    key = [pt, pt, C.neg(pt), C.INF, pts[5], pts[6]]
    for sc in ([7, 7, 0, 3, 0, 0], [9, 0, 9, 0, 4, -4], [-8, 8, 8, 1, 2, 3], [0] * 6,
               [S.INT64_MIN, (1 << 63) - 1, 1, -1, 15, -16], [8, -8, 136, -136, 120, 2184]):
        out.append(("msm 6 %s %s" % (" ".join(map(str, sc)),
                                     " ".join(C.marshal(k).hex() for k in key)),
                    C.marshal(C.commit_fast(sc, key)).hex()))
    # refused: off the curve, a coordinate >= p
    bad = bytearray(C.marshal(C.G))
    bad[40] ^= 4
    out.append(("rt " + bytes(bad).hex(), "bad"))
    out.append(("rt " + _fx(p) + _fx(2), "bad"))
    out.append(("rt " + _fx(1) + _fx((1 << 256) - 1), "bad"))
    out.append(("rt " + _fx(0) + _fx(1), "bad"))
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("commit_host")
    cs = _cases()
    path = d / "commands.txt"
    path.write_text("".join(c + "\n" for c, _ in cs))
    return d, str(path), cs


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        "-g")], ids=["plain", "sanitized"])
def test_host_program_equals_the_oracle(cases, flags):
    d, path, cs = cases
    exe = str(d / ("commit_host_" + ("san" if flags else "plain")))
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + INC,
                    *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(cs)
    for (cmd, want), g in zip(cs, got):
        assert g == want, cmd[:80]
    # the three multiplication baselines of the bench mode agree on the sum
    sums = set()
    for algo in (0, 1, 2):
        b = subprocess.run([exe, "bench", "12", "3", str(algo), "1"], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        sums.add(b.stdout.split()[1])
    assert len(sums) == 1 and sums != {C.ZERO64.hex()}
