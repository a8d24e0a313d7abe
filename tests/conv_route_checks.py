"""Which kernel family every launch of one network evaluation runs on (sgmse_amd/csrc/conv_route.h), as the engine itself names it:
``SGMSE_PROFILE_DUMP=1`` makes ``profile_forward`` print one labelled line per launch -- family, shape, and the
``+res/+gn/+shortcut/split-K/existing-tiles`` markers.  A wrong route gives a correct, slower answer, so no parity test sees it; the
listing is compared with a fixture recorded from the build BEFORE the routing moved into conv_route.h (tests/golden/conv_routes_nf128_b1.txt:
this module run as a script against that commit's tree, on an MI355X)."""
import os
import re
import subprocess
import sys

from conftest import GOLDEN, ROOT

FIXTURE = os.path.join(GOLDEN, "conv_routes_nf128_b1.txt")
SETTINGS = {"default": {}, "SGMSE_WINO43=0": {"SGMSE_WINO43": "0"}}

# the knobs are read when the engine is created: one child process per setting
_CHILD = r"""
import os, sys
root, lib, name, batch, dev, frames, tile_t = sys.argv[1:8]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'tests'))
import torch
from sgmse_amd import _lib
_lib.load_library(lib)
import parity as P
net, _ = P.make_backbone(P.NET_CASES[name], dev)
z = P.load(name)
x, t = torch.from_numpy(z['x']).repeat(1, 1, 1, int(tile_t)), torch.from_numpy(z['t'])
if frames:
    frames = [int(f) for f in frames.split(',')]
    x = [x[i % len(x), :, :, :f].contiguous().to(dev) for i, f in enumerate(frames)]
    t = t[:1].repeat(len(frames)).to(dev)
else:
    reps = (int(batch) + len(x) - 1) // len(x)
    x, t = x.repeat(reps, 1, 1, 1)[:int(batch)].contiguous().to(dev), t.repeat(reps)[:int(batch)].to(dev)
    frames = None
ctx = net.engine(torch.device(dev))
ctx.profile_forward(x, t)
print('ROUTES-DONE')
"""


def launch_labels(dev, lib, name="fwd_nf128", batch=1, env=None, frames=(), tile_t=1, root=ROOT):
    """The labels of every launch of one evaluation, times stripped, in launch order.  frames: a ragged batch of these frame counts;
    tile_t: the fixture's input repeated this many times along the frame axis."""
    out = subprocess.run([sys.executable, "-c", _CHILD, root, lib, name, str(batch), dev, ",".join(str(f) for f in frames), str(tile_t)],
                         capture_output=True, text=True, timeout=3000, env=dict(os.environ, SGMSE_PROFILE_DUMP="1", **(env or {})))
    assert "ROUTES-DONE" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    labels = [re.sub(r" [0-9.]+ ms [-0-9.a-z]+ Gwork/s$", "", ln[len("[sgmse-prof] "):])
              for ln in out.stderr.splitlines() if ln.startswith("[sgmse-prof] ")]
    assert len(labels) > 50, out.stderr[-3000:]
    return labels


def read_fixture(path=FIXTURE):
    sections, cur = {}, None
    with open(path) as f:
        for ln in f.read().splitlines():
            if ln.startswith("# "):
                cur = sections.setdefault(ln[2:], [])
            elif ln:
                cur.append(ln)
    return sections


def check_routes(dev, lib):
    want = read_fixture()
    assert set(want) == set(SETTINGS)
    for key, env in SETTINGS.items():
        got = launch_labels(dev, lib, env=env)
        fams = sorted({ln.split(" ")[0] for ln in got})
        print(f"{key}: {len(got)} launches, families {fams}")
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, want[key])) if a != b]
        assert len(got) == len(want[key]) and not diff, (key, len(got), len(want[key]), diff[:5])
    # the fixture itself shows what it is there to pin: the wide 3x3 layers on the Winograd form the setting selects
    assert any(ln.startswith("conv3x3-wino43 ") for ln in want["default"]) and not any(ln.startswith("conv3x3-wino ") for ln in want["default"])
    assert any(ln.startswith("conv3x3-wino ") for ln in want["SGMSE_WINO43=0"]) and not any(ln.startswith("conv3x3-wino43 ") for ln in want["SGMSE_WINO43=0"])


if __name__ == "__main__":      # python tests/conv_route_checks.py ROOT_OF_THE_TREE_TO_RECORD [cuda|cpu] > tests/golden/conv_routes_nf128_b1.txt
    tree = os.path.abspath(sys.argv[1])
    device = sys.argv[2] if len(sys.argv) > 2 else "cuda"
    library = os.path.join(tree, "sgmse_amd", "libsgmse_hip.so") if device == "cuda" else os.path.join(tree, "tests", "emu", "libsgmse_emu.so")
    for key, env in SETTINGS.items():
        print("# " + key)
        print("\n".join(launch_labels(device, library, env=env, root=tree)))
