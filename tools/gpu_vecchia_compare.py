"""Compare two dumps of tools/gpu_vecchia_dump.py (a parent build's and its refactoring's): the same arrays, and every one of them
bit-identical (equal bytes: NaNs and signed zeros count).  Prints one line per entry point and switch setting, then the arrays that
differ with their largest difference; exit status 1 when any does.
usage: gpu_vecchia_compare.py PARENT.npz CHILD.npz"""
import collections
import re
import sys

import numpy as np


def main(parent, child):
    P, C = np.load(parent), np.load(child)
    bad = []
    if sorted(P.files) != sorted(C.files):
        bad.append('the dumps hold different arrays: %s' % sorted(set(P.files) ^ set(C.files)))
    groups = collections.defaultdict(lambda: [0, 0, 0])   # arrays, identical, bytes
    for key in sorted(set(P.files) & set(C.files)):
        a, b = P[key], C[key]
        same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
        entry = re.search(r'(nn_ordered|nn_query|llik_batch|llik|nllik|lmatrix|het_rows|vecchia_gp|vecchia_linkgp|vpaths_nn|vpaths_rows)', key).group(1)
        g = groups[(entry, key.split('.' + entry)[0].split('.sexp')[0].split('.matern2.5')[0])]
        g[0] += 1
        g[1] += same
        g[2] += a.nbytes
        if not same:
            d = np.abs(a.astype(float) - b.astype(float)).max() if a.shape == b.shape else float('nan')
            bad.append('%s differs: max |difference| %.3g' % (key, d))
    for (entry, tag), (n, same, nbytes) in sorted(groups.items()):
        print('%-15s %-14s %4d arrays %9d bytes: %s' % (entry, tag, n, nbytes, 'bit-identical' if same == n else '%d DIFFER' % (n - same)))
    print('\n'.join(bad) if bad else 'every one of the %d arrays is bit-identical' % len(P.files))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
