"""(not gpu) Sweep 2 reads the sign words sweep 1 wrote, block by block: the sweep kernels compiled by g++ (tests/cpp/hip_shim,
as in test_sweep_emulation.py) and run on lines whose lengths straddle words and blocks -- 1 to 1024 rows, 1056 with 64-bit
entries -- with no class change, one at the first or last row of a word, at the block seams, at every row, on items that
take the fill path and items with a lane without any site.  The kernel poisons a lane's words of the scratch slot between
items and asserts at every use of a word that it is not poison (tests/cpp/sweep_sign_blocks.cc refuses to build without
assertions); the driver counts the uses and compares both passes with a brute-force line transform.  In every ring / band
size of test_sweep_emulation.py, and with blocks of one and of four words."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_sweep_emulation import CONFIGS

CPP = os.path.join(ROOT, "tests", "cpp")


# (the block size is a build knob too: one word at a time, and four)
BLOCKS = [("info1", "-DVGT_SWEEP_INFO_BLOCK=1"), ("info4", "-DVGT_SWEEP_INFO_BLOCK=4"),
          ("info4_b8", "-DVGT_SWEEP_INFO_BLOCK=4 -DVGT_SWEEP_BAND=8 -DVGT_SWEEP_RING=16 -DVGT_SWEEP_CHUNK=4")]


@pytest.mark.parametrize("name,flags", CONFIGS + BLOCKS)
def test_sign_words_in_blocks(name, flags):
    out = "sweep_sign_blocks_" + name
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "sweep_sign_blocks.mk", "BLOCKS_OUT=" + out, "SWEEP_FLAGS=" + flags])
    run = subprocess.run([os.path.join(CPP, out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    assert " 0 failures" in run.stdout
    assert "15 lengths" in run.stdout
