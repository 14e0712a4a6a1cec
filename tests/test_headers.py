"""The device headers behind csrc/hg_device.h (hg_dev_*.h, one per subject) each compile alone for the device: a
header includes what it uses, so a kernel file may include only the subjects it needs (hg_blend.hip does).  make -C
halogen-pathtracer_amd headers runs hipcc -fsyntax-only over each with the product's flags; no GPU is needed."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "halogen-pathtracer_amd"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_device_headers_compile_alone():
    if not (Path(HIPCC).exists() or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    headers = sorted(p.name for p in (PKG / "csrc").glob("hg_dev_*.h"))
    umbrella = (PKG / "csrc" / "hg_device.h").read_text()
    assert headers and all(f'#include "{h}"' in umbrella for h in headers), headers
    r = subprocess.run(["make", "-s", "-C", str(PKG), "headers", f"HIPCC={HIPCC}"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
