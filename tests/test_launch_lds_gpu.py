"""isic_launch_lds (csrc/common.h) opts a kernel into its largest dynamic LDS size once per device and process.  The
entries that used to set the attribute on every launch -- the attention pools and the row-tile k-NN kernel -- are driven
through small, large, largest and small sizes again in a fresh process (tests/launch_lds_child.py has the cases, the byte
counts and the references), where the first launch of each kernel is the one that sets the attribute."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_kernels_take_every_lds_size_after_the_one_time_opt_in():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_lds_child.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("LAUNCH_LDS_OK"), r.stdout[-3000:]
    assert r.stdout.count(" refused") == 4, r.stdout[-3000:]
