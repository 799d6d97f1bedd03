"""GPU: the frame's local-map chain (tests/localmap_chain.py) — spfe_update_local_map_resident, spfe_gather_map_points_device with
n = point_cap, spfe_track_local_map_record_device with n = point_cap on a real record, spfe_local_map_rows_resident — on ONE
stream with nothing read back in between, against the host-driven route (the list of tests/localmap_ref/localmap_ref.c with the
exact n_points, uploaded): the pose block, the frame's holders as list positions and as table rows, and the search outputs of the
first n_points points are equal, and no padding row of the list is matched.  Then the same chain captured into a hipGraph and
replayed on a second input: the capture-and-replay test of the four entry points whose names end in _resident (the table of
tests/graph_forms.py is closed at the 37 *_device forms), with that table's sequence and safety rule — the direct calls first
(the only size there is, so the first sizes every scratch), one fresh process, one verdict line.  The record is one of the
240 x 320 scene the extents tests track on."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_chain_equals_the_host_route_and_replays_from_a_graph():
    r = subprocess.run([sys.executable, "-m", "tests.localmap_chain"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    verdict = [line for line in r.stdout.splitlines() if line.startswith("local-map chain: ")]
    print(out[-4000:])
    assert r.returncode == 0, verdict or out[-2000:]
    assert len(verdict) == 1 and verdict[0].startswith("local-map chain: PASS kernel=14 memset=0"), verdict
