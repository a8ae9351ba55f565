"""SHA-1 of the gfx950 code object of every translation unit in two builds of libdgp_amd.so, side by side: a change that is meant to leave the
device code alone (host-side refactoring, deleted dead variants) must give the same bytes, unit by unit.  No GPU needed.
usage: code_objects.py OTHER/libdgp_amd.so [THIS/libdgp_amd.so]      (exit status 1 when a unit differs)"""
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_isa_hazards import device_objects, LIB   # noqa: E402

units = sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, 'dgp_amd', 'csrc', '*.hip')))   # the Makefile's link order
a, b = (device_objects(p) for p in (sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else LIB))
assert len(a) == len(b) == len(units), (len(a), len(b), len(units))
same = True
print('%-20s %9s %-40s %9s %-40s' % ('translation unit', 'bytes', 'SHA-1 (other)', 'bytes', 'SHA-1 (this)'))
for u, x, y in zip(units, a, b):
    print('%-20s %9d %-40s %9d %-40s %s' % (u, len(x), hashlib.sha1(x).hexdigest(), len(y), hashlib.sha1(y).hexdigest(), 'same' if x == y else 'DIFFERENT'))
    same &= x == y
sys.exit(0 if same else 1)
