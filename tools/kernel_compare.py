"""Kernel by kernel, two builds of libdgp_amd.so whose translation units differ (a file was split or merged): for every kernel of the
gfx950 code objects its registers, scratch, static LDS and occupancy from the code object's notes and its instruction text from the
disassembly, side by side.  Branch targets and the addresses inside <...> are dropped from the text (a kernel that moved to another
code object keeps its instructions, not its addresses).  Code objects that are byte-identical in both builds are counted, not
listed.  No GPU needed.
usage: kernel_compare.py OTHER/libdgp_amd.so [THIS/libdgp_amd.so]      (exit status 1 when a kernel differs)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_isa_hazards import device_objects, LIB, OBJDUMP   # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), 'llvm-readelf')
FIELDS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'max_flat_workgroup_size',
          'vgpr_spill_count', 'sgpr_spill_count')


def occupancy(k):
    """waves per SIMD by registers alone: the unified file of gfx950 has 512 per lane, allocated in eights (vgpr_count is the
    unified total, AGPRs included), at most 8 waves"""
    return min(8, 512 // max(-(-k['vgpr_count'] // 8) * 8, 8))


def kernels(obj, tmp):
    f = os.path.join(tmp, 'dev.o')
    open(f, 'wb').write(obj)
    notes = subprocess.run([READELF, '--notes', f], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in re.split(r'\n\s*- \.agpr_count:', notes)[1:]:
        blk = '.agpr_count:' + blk
        k = {fld: int(re.search(r'\.%s:\s*(\d+)' % fld, blk).group(1)) for fld in FIELDS}
        out[re.search(r'\.symbol:\s*(\S+)\.kd', blk).group(1)] = k
    txt = subprocess.run([OBJDUMP, '-d', '--mcpu=gfx950', '--no-show-raw-insn', f], capture_output=True, text=True, check=True).stdout
    for m in re.finditer(r'^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)', txt, re.S | re.M):
        if m.group(1) not in out:
            continue
        ins = [ln.split('//')[0].strip() for ln in m.group(2).splitlines() if ln.strip() and not ln.strip().startswith(';')]
        ins = [re.sub(r'^(s_c?branch\S*).*', r'\1', re.sub(r'\s*<[^>]*>', '', i)) for i in ins if i != '...']
        for at, i in enumerate(ins):   # (s_getpc_b64, then s_add_u32 / s_addc_u32 of a pc-relative distance: to a table in .rodata)
            if i.startswith('s_getpc_b64'):
                ins[at + 1:at + 3] = [re.sub(r'0x[0-9a-f]+$', 'REL', j) for j in ins[at + 1:at + 3]]
        while ins and ins[-1].split()[0] in ('s_nop', 's_code_end'):   # (padding behind s_endpgm: to the next kernel's alignment, at the end of .text)
            ins.pop()
        out[m.group(1)].update(instructions=len(ins), text=hashlib.sha1('\n'.join(ins).encode()).hexdigest()[:12], ins=ins)
    return out


def library(path, skip):
    with tempfile.TemporaryDirectory() as tmp:
        ks = {}
        for obj in device_objects(path):
            if hashlib.sha1(obj).digest() not in skip:
                ks.update(kernels(obj, tmp))
        return ks


pa, pb = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else LIB
ha, hb = ({hashlib.sha1(o).digest() for o in device_objects(p)} for p in (pa, pb))
print('code objects: %d (other), %d (this), %d byte-identical in both; the kernels of the rest:' % (len(ha), len(hb), len(ha & hb)))
a, b = library(pa, ha & hb), library(pb, ha & hb)
same = True
print('%-62s %5s %5s %5s %8s %7s %4s %6s %-12s' % ('kernel', 'vgpr', 'agpr', 'sgpr', 'scratch', 'LDS', 'occ', 'instr', 'text sha1'))
for name in sorted(set(a) | set(b)):
    for tag, ks in (('other', a), ('this', b)):
        k = ks.get(name)
        if k:
            print('%-56s %-5s %5d %5d %5d %8d %7d %4d %6d %-12s' % (name[:56], tag, k['vgpr_count'], k['agpr_count'], k['sgpr_count'],
                  k['private_segment_fixed_size'], k['group_segment_fixed_size'], occupancy(k), k['instructions'], k['text']))
        else:
            print('%-56s %-5s absent' % (name[:56], tag))
    x, y = a.get(name), b.get(name)
    if not (x and y):
        same = False
        continue
    res = all(x[f] == y[f] for f in FIELDS)
    verdict = 'resources %s, text %s' % ('equal' if res else 'DIFFERENT', 'identical' if x['text'] == y['text'] else 'DIFFERENT')
    if x['text'] != y['text']:
        mx, my = ([i.split()[0] for i in k['ins']] for k in (x, y))
        verdict += ' (%s)' % ('the same mnemonics in the same order: registers or immediates differ' if mx == my else
                              'the same multiset of mnemonics in another order' if sorted(mx) == sorted(my) else 'other instructions')
        same = False
    same &= res
    print('    ' + verdict)
sys.exit(0 if same else 1)
