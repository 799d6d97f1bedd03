"""GPU: a keyframe insertion as one captured graph (tests/covis_chain.py) — spfe_covis_reset_slots_resident for the new slot,
spfe_update_connections_resident, spfe_detect_loop_candidates_device taking its 10-column table, d_connected and d_covisible
straight from the graph state, spfe_update_local_map_resident taking the 20-column table and d_parent from it — on ONE stream with
nothing read back in between: the three blocks, all eight state arrays and both tables equal the three host references chained in
Python (tests/covis_ref, tests/loopdet_ref, tests/localmap_ref).  Then the same four calls captured into a hipGraph, for one
keyframe and for the next: no memset node, 16 kernel nodes each, replayed on a second input and on the second keyframe (on the
state the first replay left on the device).  One fresh process, one verdict line, the direct calls first; the process's hardware
queue count is left as the machine sets it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_insertion_equals_the_host_references_and_replays_from_a_graph():
    r = subprocess.run([sys.executable, "-m", "tests.covis_chain"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    verdict = [line for line in r.stdout.splitlines() if line.startswith("covisibility chain: ")]
    print(out[-4000:])
    assert r.returncode == 0, verdict or out[-2000:]
    assert len(verdict) == 1 and verdict[0].startswith("covisibility chain: PASS kernel=16+16 memset=0"), verdict
