"""CPU pin of the STRING-key hash spec (distributed_join_amd/csrc/dj_strhash.h).

A stand-alone C program (its own main, nothing preloaded, nothing loaded
into Python) includes the header, copies every vector of
tests/golden/murmur3_public_vectors.json into an exact-size heap buffer,
and prints dj_murmur3_bytes for the vector's seed plus both halves of
dj_string_key64. The PUBLISHED hashes in the fixture decide; where the host
compiler can link -fsanitize=address,undefined the program runs under it, so
a read outside p[0..len) aborts the run.
"""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "murmur3_public_vectors.json")
CSRC = os.path.join(REPO, "distributed_join_amd", "csrc")

PROGRAM = r"""
#include "dj_strhash.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* argv: pairs of <hex bytes or "-" for empty> <seed hex> */
int main(int argc, char** argv)
{
  for (int i = 1; i + 1 < argc; i += 2) {
    const char* hex = argv[i];
    int32_t len = strcmp(hex, "-") == 0 ? 0 : (int32_t)(strlen(hex) / 2);
    /* exact-size heap buffer: one byte past the end is out of bounds */
    uint8_t* buf = len ? (uint8_t*)malloc((size_t)len) : NULL;
    for (int32_t k = 0; k < len; k++) {
      unsigned v;
      sscanf(hex + 2 * k, "%2x", &v);
      buf[k] = (uint8_t)v;
    }
    uint32_t seed = (uint32_t)strtoul(argv[i + 1], NULL, 16);
    uint64_t k64 = dj_string_key64(buf, len);
    printf("%08x %08x %08x\n", dj_murmur3_bytes(buf, len, seed),
           (uint32_t)(k64 & 0xFFFFFFFFu), (uint32_t)(k64 >> 32));
    free(buf);
  }
  return 0;
}
"""


def _vectors():
    with open(GOLDEN) as fh:
        fixture = json.load(fh)
    out = []
    for vec in fixture["vectors"]:
        data = (bytes.fromhex(vec["data_hex"]) if "data_hex" in vec
                else vec["data_utf8"].encode())
        out.append((data, int(vec["seed"], 16), int(vec["hash"], 16)))
    return out


def _can_link(cc, flags, tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    exe = tmp_path / "probe"
    r = subprocess.run([cc, *flags, str(probe), "-o", str(exe)], capture_output=True)
    return r.returncode == 0 and subprocess.run([str(exe)], capture_output=True).returncode == 0


def test_strhash_public_vectors(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no host C compiler"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    flags = san if _can_link(cc, san, tmp_path) else []
    src = tmp_path / "strhash_vectors.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "strhash_vectors"
    r = subprocess.run([cc, "-std=c99", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC,
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    vectors = _vectors()
    assert len(vectors) >= 13
    args = []
    for data, seed, _ in vectors:
        args += [data.hex() or "-", "%08x" % seed]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split()
    got = [tuple(int(x, 16) for x in lines[3 * i:3 * i + 3]) for i in range(len(vectors))]

    # published hash per (data, seed)
    published = {(data, seed): want for data, seed, want in vectors}
    halves_checked = 0
    for (data, seed, want), (h, lo, hi) in zip(vectors, got):
        assert h == want, (data, hex(seed), hex(h), hex(want))
        # dj_string_key64 = murmur3(seed 0) | murmur3(seed 0x9747B28C) << 32:
        # each half against the published vector of that seed, where present
        if (data, 0) in published:
            assert lo == published[(data, 0)], (data, hex(lo))
            halves_checked += 1
        if (data, 0x9747B28C) in published:
            assert hi == published[(data, 0x9747B28C)], (data, hex(hi))
            halves_checked += 1
    assert halves_checked >= 10
