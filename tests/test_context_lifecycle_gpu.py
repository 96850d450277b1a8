"""Life cycle of a context's device resources: every device buffer, pinned buffer, stream and event a context makes belongs to an
owner inside it (radiativetransfer_amd/csrc/ftte_device.h), and ftte_counter "device_objects" counts the owned objects alive in the
process.  tests/context_lifecycle_child.py, in a process of its own, drives a context three times over through uniform brick
sweeps with a growing and then a smaller number of frequency groups (once with emission), a refined cell array swept by the hybrid
sweep with a fine block and by the segment forests alone, a point-source trace on a medium, the equilibrium update and the
hydrogen census, ftte_diffuse_iteration with pageable host arrays, and a different uniform grid; destroys it and makes a fresh one.
The fresh context reports the count the first one started with each time, J of the first uniform sweep is the same in the third
round as in the first, bit for bit, and a context on devices [0, 0] passes the same once."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_a_destroyed_context_leaves_nothing_and_a_fresh_one_computes_the_same():
    run = subprocess.run([sys.executable, os.path.join(HERE, "context_lifecycle_child.py")], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "context lifecycle OK" in run.stdout, (run.stdout + run.stderr)[-4000:]
