"""Static instruction mix of one kernel in a gfx950 ISA listing (hipcc
--save-temps .s): fp64 VALU against integer / select / move VALU, SALU, LDS
and global memory instructions, and the kernel's register and LDS use.
usage: isa_mix.py file.s name-substring [name-substring ...] (all must match)"""
import re
import sys
from collections import Counter

s = open(sys.argv[1]).read()
keys = sys.argv[2:]
m = [mm for mm in re.finditer(r'^(_Z\S+):', s, re.M) if all(k in mm.group(1) for k in keys)][0]
name = m.group(1)
start = m.end()
end = s.index('.Lfunc_end', start)
c = Counter()
for ln in s[start:end].split('\n'):
    t = ln.strip()
    if not t or t[0] in ';.' or t.endswith(':'):
        continue
    op = t.split()[0]
    if op.startswith('v_'):
        if op.endswith('_f64') or '_f64_' in op:
            c['valu_fp64'] += 1
        elif op.startswith('v_cndmask'):
            c['valu_select'] += 1
        elif op.startswith(('v_mov', 'v_accvgpr', 'v_readfirstlane', 'v_readlane', 'v_writelane')):
            c['valu_move'] += 1
        elif op.startswith('v_cmp'):
            c['valu_compare'] += 1
        else:
            c['valu_int_other'] += 1
        c['valu'] += 1
    elif op.startswith(('global_load', 'buffer_load')):
        c['vmem_read'] += 1
    elif op.startswith(('global_store', 'buffer_store')):
        c['vmem_write'] += 1
    elif op.startswith('ds_'):
        c['lds'] += 1
    elif op == 's_barrier':
        c['barrier'] += 1
    elif op.startswith('s_waitcnt'):
        c['waitcnt'] += 1
    elif op.startswith('scratch'):
        c['scratch'] += 1
    elif op.startswith('s_'):
        c['salu'] += 1
print(name)
for k in ('valu', 'valu_fp64', 'valu_int_other', 'valu_select', 'valu_move', 'valu_compare', 'salu', 'lds', 'vmem_read',
          'vmem_write', 'barrier', 'waitcnt', 'scratch'):
    print(f"  {k:16s} {c[k]:6d}")
tail = s[end:end + 6000]  # the resource comment block that follows the kernel
for mm in re.finditer(r'^; (NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize): (.*)$', tail, re.M):
    print(f"  {mm.group(1):16s} {mm.group(2)}")
