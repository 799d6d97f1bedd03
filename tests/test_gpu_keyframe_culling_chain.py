"""GPU: the tail of a mapping cycle as one captured graph (tests/cull_chain.py) — spfe_count_observations_resident,
spfe_cull_keyframes_resident, spfe_update_connections_resident of the NEXT keyframe on the rows, flags and graph the cull left,
and spfe_update_local_map_resident reading its table, d_parent and the flags with the cull's new bits — on ONE stream with nothing
read back in between: the three blocks, the rows, both flag arrays, the observation counts, all eight state arrays and both tables
equal the host references chained in Python (tests/cull_ref, tests/covis_ref, tests/localmap_ref).  Then the same four calls
captured into a hipGraph: no memset node, 18 kernel nodes (2 + 4 + 5 + 7), replayed on a second input and on the first again.  One
fresh process, one verdict line, the direct calls first; the process's hardware queue count is left as the machine sets it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_cycle_tail_equals_the_host_references_and_replays_from_a_graph():
    r = subprocess.run([sys.executable, "-m", "tests.cull_chain"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    verdict = [line for line in r.stdout.splitlines() if line.startswith("keyframe culling chain: ")]
    print(out[-4000:])
    assert r.returncode == 0, verdict or out[-2000:]
    assert len(verdict) == 1 and verdict[0].startswith("keyframe culling chain: PASS kernel=18 memset=0"), verdict
