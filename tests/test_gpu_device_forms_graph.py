"""GPU: every *_device form of include/spfe.h other than spfe_extract_batch_device captured into a hipGraph and replayed on
other inputs (tests/graph_forms.py has the table, the sequence and the safety rule): "N launches on `stream`, no host
synchronisation, no host decision; scratch is allocated before the first launch".  One fresh process per form, so that a refused
or invalidated capture cannot poison the next case; the process prints one verdict line and exits 0 or 1."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_forms  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(graph_forms.FORMS))
def test_one_captured_call_replays_on_other_inputs_byte_for_byte(name):
    r = subprocess.run([sys.executable, "-m", "tests.graph_forms", name], cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    verdict = [line for line in r.stdout.splitlines() if line.startswith("graph-form %s: " % name)]
    print(out[-4000:])
    assert r.returncode == 0, verdict or out[-2000:]
    assert len(verdict) == 1 and verdict[0].startswith("graph-form %s: PASS kernel=" % name), verdict
