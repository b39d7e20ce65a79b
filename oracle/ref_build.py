"""Builds the reference-side proof executables into oracle/_ref/ (build products, kept out of git).

The reference checkout (read-only; $VQVDB_REFERENCE, or found by tools/prove_integration.py's find_reference()) is read here,
at build time only: tools/prove_integration.py --build compiles INTEGRATION.md §2/§3 applied to temporary copies of the reference's
factory and SOP statements, and a leaf_harness whose embedded pack header comes from the reference's own generator.  The tests run
these executables and never read the reference themselves.  Without a reference checkout nothing is built."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
OUT = os.path.join(_HERE, "_ref", "integration")


def build() -> str | None:
    """Returns the output directory, or None when there is no reference checkout to build from."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_integration
    if not os.path.isdir(prove_integration.REF):
        return None
    shutil.rmtree(OUT, ignore_errors=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prove_integration.py"), "--build", OUT], cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        shutil.rmtree(OUT, ignore_errors=True)
        raise RuntimeError("building the reference-side proof executables failed:\n" + (r.stdout + r.stderr)[-4000:])
    return OUT
