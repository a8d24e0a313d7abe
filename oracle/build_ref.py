"""Recipe of ``oracle/_ref/`` (called by ``__graft_entry__.build()``; the directory is never committed).

The one piece of the upstream tree a test runs as it is: its ``enhancement.py``, copied byte for byte, which
``tests/parity.py::check_reference_script_unmodified`` executes on top of this package.  The upstream tree is looked up
as the golden-fixture scripts do (``SGMSE_REFERENCE``; ``SGMSE_REFERENCE_DIR`` is accepted too), falling back to
BASELINE.json's ``reference_path``.  Where the tree is absent nothing is copied and that test skips.
"""
import json
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
SCRIPTS = ("enhancement.py",)


def reference_dir():
    env = os.environ.get("SGMSE_REFERENCE_DIR") or os.environ.get("SGMSE_REFERENCE")
    if env:
        return env
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as fh:
            return json.load(fh).get("reference_path")
    except (OSError, ValueError):
        return None


def build():
    """Copies the upstream scripts into oracle/_ref/; returns the list of what was copied (empty without the tree)."""
    ref = reference_dir()
    done = []
    for name in SCRIPTS:
        src = os.path.join(ref, name) if ref else None
        if not src or not os.access(src, os.R_OK):
            continue
        os.makedirs(REF_OUT, exist_ok=True)
        shutil.copyfile(src, os.path.join(REF_OUT, name))
        done.append(name)
    return done


if __name__ == "__main__":
    print("oracle/_ref:", build() or "no upstream tree found, nothing copied")
