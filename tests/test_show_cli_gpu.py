"""The CLI's ``--show N --mark`` on the device: Hamlet's ``to be`` phrase, and the same ranked
under ``--ignore-case``; each equals the oracle's formatting and ``--backend cpu``."""
import os
import subprocess

import pytest

from tests.show_cases import formatted_show, want_show

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shown(out: bytes) -> bytes:
    """The result lines: every query's line and the shown lines under it."""
    keep = [l for l in out.split(b"\n") if l.startswith(b"print query:") or l.startswith(b"  ")]
    return b"".join(l + b"\n" for l in keep)


@pytest.mark.parametrize("extra, k, fold", [([], None, False),
                                             (["--rank", "3", "--ignore-case"], 3, True)])
def test_cli_show_mark(cli, hamlet, extra, k, fold):
    args = ["data/hamlet.txt", "--search", "to be", "--match", "phrase", "--show", "80", "--mark",
            "--check", *extra]
    gpu = subprocess.run([cli, *args], capture_output=True, timeout=100, cwd=ROOT)
    assert gpu.returncode == 0, gpu.stderr.decode()[-2000:]
    cpu = subprocess.run([cli, *args, "--backend", "cpu"], capture_output=True, timeout=100, cwd=ROOT)
    assert cpu.returncode == 0, cpu.stderr.decode()[-2000:]
    queries = [[b"to", b"be"]]
    expect = want_show(hamlet, queries, "phrase", 80, k, ignore_case=fold)
    want_out = formatted_show(queries, expect, k, mark=True)
    assert b">>to<< >>be<<" in want_out or b">>To<< >>be<<" in want_out
    assert gpu.stdout.count(want_out) == 1
    assert shown(gpu.stdout) == shown(cpu.stdout)
