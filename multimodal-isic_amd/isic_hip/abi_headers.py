"""The one list of opt-in ABI headers: the ``#include "isic_hip_*.h"`` lines of ``include/isic_hip.h``.

Standard library only, so that ``build.py`` can read the list before the shared library exists; ``lib.py`` binds the
entry points of the same headers.  A new kernel family adds its header with one ``#include`` line and nothing else."""
from __future__ import annotations

import os
import re

_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"(isic_hip_\w+\.h)"', re.M)


def included_headers(isic_hip_h):
    """Paths of the headers ``isic_hip_h`` includes from its own directory, in the order of its ``#include`` lines."""
    with open(isic_hip_h) as f:
        names = _INCLUDE.findall(f.read())
    inc = os.path.dirname(isic_hip_h)
    return [os.path.join(inc, n) for n in names]
