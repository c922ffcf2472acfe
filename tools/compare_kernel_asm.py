"""Compare the kernels of two hipcc gfx950 assembly files (the -save-temps .s of two builds of one source), symbol by symbol.

For every kernel (.amdgpu_metadata entry) of either file: whether its instruction stream -- labels, comments and directives
stripped -- is the same in both, and for one that differs the figures that decide its occupancy class, old -> new: vgpr_count,
sgpr_count, group_segment_fixed_size, private_segment_fixed_size and the instruction count.  Reads nothing but the two files.
A refactor that claims to leave code generation alone shows `identical` on every line.
--may-differ=SUBSTRING: kernels whose name contains SUBSTRING are the ones under change; with --fail the exit code is 1 when
any OTHER kernel differs or is missing on one side, or when a differing kernel has scratch (private segment) in the new file.
usage: python tools/compare_kernel_asm.py old.s new.s [--may-differ=SUBSTRING ...] [--fail]"""
import re
import sys

FIELDS = ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')


def kernels(path):
    """name -> (instruction list, metadata dict)"""
    code, cur, meta, entry, in_meta = {}, None, {}, None, False
    for line in open(path):
        if line.startswith('\t.amdgpu_metadata') or line.startswith('.amdgpu_metadata'):
            in_meta = True
            continue
        if in_meta:
            m = re.match(r'  (- |  )\.(\w+):\s*(\S.*)?$', line)        # a kernel's own keys: the argument lists sit deeper
            if not m:
                continue
            if m.group(1) == '- ':
                entry = {}
            if entry is not None:
                entry[m.group(2)] = (m.group(3) or '').strip()
                if m.group(2) == 'name':
                    meta[entry['name']] = entry
            continue
        s = line.split(';')[0].split('//')[0].strip()
        if not s:
            continue
        head = s.split()[0]
        if head.endswith(':'):
            if not head.startswith(('.', 'BB')):
                cur = code.setdefault(head[:-1], [])
            continue
        if s.startswith('.'):
            if s.startswith(('.end_amdhsa_kernel', '.section', '.text')):
                cur = None
            continue
        if cur is not None:
            cur.append(s)
    out = {}
    for name, entry in meta.items():
        if name in code and 'vgpr_count' in entry:
            out[name] = (code[name], {k: int(entry.get(k, -1)) for k in FIELDS})
    return out


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith('--')]
    may = [a.split('=', 1)[1] for a in sys.argv[1:] if a.startswith('--may-differ=')]
    old, new = kernels(paths[0]), kernels(paths[1])
    bad = same = 0
    for name in sorted(set(old) | set(new)):
        free = any(s in name for s in may)
        if name not in old or name not in new:
            print('%-9s %s' % ('only old' if name in old else 'only new', name))
            bad += 1
            continue
        (ci, mi), (cj, mj) = old[name], new[name]
        if ci == cj and mi == mj:
            same += 1
            print('%-9s %s  (%d instructions, %d vgpr, %d B lds)' % ('identical', name, len(ci), mi['vgpr_count'], mi['group_segment_fixed_size']))
            continue
        print('%-9s %s' % ('DIFFERS', name))
        print('          instructions %d -> %d' % (len(ci), len(cj)))
        for k in FIELDS:
            print('          %s %d -> %d' % (k, mi[k], mj[k]))
        if not free or mj['private_segment_fixed_size'] != 0:
            bad += 1
    print('%d kernels, %d identical' % (len(set(old) | set(new)), same))
    sys.exit(1 if bad and '--fail' in sys.argv else 0)


if __name__ == '__main__':
    main()
