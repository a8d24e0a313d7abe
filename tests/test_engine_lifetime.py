"""The engine's memory management under AddressSanitizer: tests/emu/engine_lifetime_main.cpp, a stand-alone program over the CPU
emulator runtime, walks every path of sgmse::Engine that allocates, grows, re-allocates or releases a buffer (and one that throws
with scratch alive) and destroys the engine.  It runs in its own process; nothing of it is loaded into this one."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.slow
@pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="minutes of compilation under the sanitizer, then ~1.5 min on the emulator; set SGMSE_SLOW=1")
def test_engine_lifetime_under_address_sanitizer():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sgmse_amd", "csrc"), "lifetime"])
    r = subprocess.run([os.path.join(ROOT, "tests", "emu", "engine_lifetime")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=1800)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]      # (a sanitizer report, invalid access or leak at exit, ends the program with a non-zero status)
    assert "Sanitizer" not in r.stdout and "[lifetime] done" in r.stdout, r.stdout[-4000:]
