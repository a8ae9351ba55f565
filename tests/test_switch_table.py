"""The DGPAMD_* environment switches: one table in csrc/context.hip (read by dgpamd_create, nowhere else in the C library), the os.environ reads of
dgp_amd/*.py, and ONE documented list of both in INTEGRATION.md.  No GPU: this reads the sources."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dgp_amd', 'csrc')
NAME = r'DGPAMD_[A-Z0-9_]+'


def read(path):
    with open(path, errors='replace') as f:
        return f.read()


def documented():
    """first column of the switch table of INTEGRATION.md"""
    return set(re.findall(r'^\| `(%s)` \|' % NAME, read(os.path.join(ROOT, 'INTEGRATION.md')), re.M))


def read_by_the_library():
    c = set(re.findall(r'\{"(%s)", &Tuning::' % NAME, read(os.path.join(CSRC, 'context.hip'))))
    py = set()
    for f in glob.glob(os.path.join(ROOT, 'dgp_amd', '*.py')):
        py |= set(re.findall(r'''environ(?:\.get\(|\[)\s*['"](%s)['"]''' % NAME, read(f)))
    return c, py


def test_every_switch_read_is_documented_and_nothing_else():
    c, py = read_by_the_library()
    assert len(c) == 25 and len(py) == 15 and 'DGPAMD_LIB' in py, (sorted(c), sorted(py))
    assert c | py == documented(), sorted((c | py) ^ documented())


def test_only_context_hip_reads_the_environment():
    for f in sorted(glob.glob(os.path.join(CSRC, '*'))):
        if os.path.basename(f) != 'context.hip' and os.path.isfile(f) and not f.endswith(('.o', '.so')):
            assert 'getenv' not in read(f), f
    assert read(os.path.join(CSRC, 'context.hip')).count('getenv(') == 1   # (the walk over the table in dgpamd_create)


def test_tests_and_tools_set_only_switches_that_exist():
    """a switch that tests/ or tools/ set (environment assignment, dictionary entry, keyword of a helper, shell prefix) is in the table"""
    known = documented()
    assert known
    setters = (r'''(%s)['"]\s*\]\s*=''', r'''['"](%s)['"]\s*:''', r'''setenv\(\s*['"](%s)['"]''', r'''\b(%s)=''', r'''export\s+(%s)\b''')
    for d in ('tests', 'tools'):
        for f in sorted(glob.glob(os.path.join(ROOT, d, '*'))):
            if not f.endswith(('.py', '.sh')):
                continue
            txt = read(f)
            used = set()
            for pat in setters:
                used |= set(re.findall(pat % NAME, txt))
            # (tests/test_gpu_ops.py names them without the prefix: engine_under(NAME=value), {'NAME': value} passed to it)
            if os.path.basename(f) == 'test_gpu_ops.py':
                for call in re.findall(r'engine_under\(([^)]*)\)', txt):
                    used |= {'DGPAMD_' + k for k in re.findall(r'\b([A-Z][A-Z0-9_]+)=', call)}
                for block in re.findall(r'for env in \((.*?)\):\n', txt, re.S):
                    used |= {'DGPAMD_' + k for k in re.findall(r"'([A-Z][A-Z0-9_]+)':", block)}
            assert used <= known, (f, sorted(used - known))
