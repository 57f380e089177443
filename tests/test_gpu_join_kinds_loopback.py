"""Left / left semi / left anti joins across several ranks: G ranks as threads
over a counting loopback Communicator (tests/cpp/joinkinds_loopback.cpp),
every result against a host join of the global tables; the semi join's wire
bytes do not depend on the right table's payload columns."""
import subprocess

import pytest

import cpp_programs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    import distributed_join_amd as dj
    dj.require_gpu()
    return cpp_programs.build("joinkinds_loopback")


@pytest.mark.parametrize("G", [2, 3, 8])
def test_join_kinds_loopback(exe, G):
    r = subprocess.run([exe, str(G), "1000"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("JOIN KINDS LOOPBACK OK") == 1, r.stdout
    runs = [l for l in r.stdout.splitlines() if " host rows=" in l]
    # 3 kinds x 2 key settings, 2 unmatched-null-key runs, 2 wire-byte runs,
    # and the inter-domain run at G = 8
    assert len(runs) == (11 if G == 8 else 10), r.stdout
