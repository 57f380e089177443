"""null_equality::UNEQUAL across several ranks: G ranks as threads over the
counting loopback Communicator (tests/cpp/nullequality_loopback.cpp). Every
kind against the host join of the globally stripped tables plus the stripped
left rows (LEFT, LEFT_ANTI); the Mailbox sees the sends and bytes of the EQUAL
join of tables the host stripped beforehand, so null-key rows never reach the
communicator, whatever they carry."""
import subprocess

import pytest

import cpp_programs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    import distributed_join_amd as dj
    dj.require_gpu()
    return cpp_programs.build("nullequality_loopback")


@pytest.mark.parametrize("G", [2, 3, 8])
def test_null_equality_loopback(exe, G):
    r = subprocess.run([exe, str(G), "1000"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("NULL EQUALITY LOOPBACK OK") == 1, r.stdout
    runs = [l for l in r.stdout.splitlines() if " host rows=" in l]
    # 4 kinds x (UNEQUAL, EQUAL on pre-stripped tables), 2 x 2 runs whose
    # null-key right rows differ, and the inter-domain pair at G = 8
    assert len(runs) == (14 if G == 8 else 12), r.stdout
