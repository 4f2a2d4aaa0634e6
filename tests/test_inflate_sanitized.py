"""csrc/sg_inflate.h -- the decode core the device kernel runs -- on the host, as a stand-alone program (tests/tools/inflate_check.cpp,
its own ``main``), under the address and undefined-behaviour sanitizers where they can be had, over every valid and every corrupt
stream of tests/unpng_case.py: the program's status and the hash of what it produced must be the Python restatement's
(``unpng.inflate_host``), and a sanitized build must have nothing to say.  The streams the device is given in tests/test_gpu_unpng.py
are these same ones; here the core reads every one of them inside an allocation of exactly its size.

The program is built with ``-fsanitize=address,undefined`` where the compiler links that, plainly otherwise (the first test prints which
build ran); it runs as a child process, nothing is preloaded, nothing of it touches a GPU."""
import os
import shutil
import subprocess

import pytest

import unpng_case as uc
from sings_amd import unpng as U

_BUILT = {}


def _program(repo_root, tmp):
    """-> (path, sanitized?) of the built program; built once per process."""
    if not _BUILT:
        cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
        assert cxx, "no C++ compiler for the host check of csrc/sg_inflate.h"
        src, exe = os.path.join(repo_root, "tests", "tools", "inflate_check.cpp"), os.path.join(tmp, "inflate_check")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, src]
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        # (the runtimes inside the program where the compiler can: it then needs nothing of its environment)
        for flags in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
            r = subprocess.run(base + flags, capture_output=True, text=True)
            if r.returncode == 0:
                break
        sanitized = bool(flags)
        assert r.returncode == 0, r.stderr
        _BUILT["program"] = (exe, sanitized)
    return _BUILT["program"]


@pytest.fixture(scope="module")
def program(repo_root, tmp_path_factory):
    return _program(repo_root, str(tmp_path_factory.mktemp("inflate_check")))


def _run(program, tmp_path, streams):
    """[(stream, expected)] -> [(status, produced, hash)] by one child process."""
    args = []
    for i, (stream, expected) in enumerate(streams):
        path = os.path.join(str(tmp_path), f"{i}.z")
        with open(path, "wb") as f:
            f.write(stream)
        args += [path, str(expected)]
    r = subprocess.run([program[0]] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(streams)
    return [(int(a), int(b), int(c, 16)) for a, b, c in (line.split() for line in lines)]


def test_the_core_on_the_host_gives_the_twins_status_and_bytes_on_every_valid_stream(program, tmp_path):
    print("sanitized build:", program[1])
    twins = [uc.twin_valid(name) for name, _ in uc.VALID]
    got = _run(program, tmp_path, [(t[3], t[1] * (1 + t[0] * t[2])) for t in twins])
    for (name, _), t, g in zip(uc.VALID, twins, got):
        assert g == (t[5], len(t[4]), uc.fnv(t[4])) and g[0] == 0, name


def test_the_core_on_the_host_gives_the_twins_status_on_every_corrupt_stream(program, tmp_path):
    W, H, ch = uc.CORRUPT_SHAPE
    expected = H * (1 + W * ch)
    got = _run(program, tmp_path, [(c[1], expected) for c in uc.CORRUPT])
    for (name, stream, named, _), g in zip(uc.CORRUPT, got):
        raw, status = U.inflate_host(stream, expected)
        assert g == (status, len(raw), uc.fnv(raw)), name
        assert g[0] == (named if named != U.E_FILTER else 0), name             # (a filter byte is not the inflate's business)


def test_the_core_on_the_host_survives_every_truncation_and_every_flipped_bit_of_a_small_stream(program, tmp_path):
    """Beyond the named cases: a dynamic-code stream cut at every length, and with every bit of its first 48 bytes (the block header and
    the code lengths) flipped.  Whatever the status, it is the twin's, and the sanitizers stay silent."""
    W, H, ch, stream, raw, _ = uc.twin_valid("zlib-21x13x3-level9")
    expected = len(raw)
    assert stream[2] & 6 == 4, "a dynamic block first"
    streams = [stream[:n] for n in range(len(stream))]
    for bit in range(16, 48 * 8):
        s = bytearray(stream)
        s[bit // 8] ^= 1 << (bit % 8)
        streams.append(bytes(s))
    got = _run(program, tmp_path, [(s, expected) for s in streams])
    seen = set()
    for s, g in zip(streams, got):
        r, status = U.inflate_host(s, expected)
        assert g == (status, len(r), uc.fnv(r)), len(s)
        seen.add(status)
    assert 0 not in {g[0] for g in got[:len(stream)]} and len(seen) >= 6, seen
