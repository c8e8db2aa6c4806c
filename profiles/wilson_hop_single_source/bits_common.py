"""What the three comparison scripts of this folder share: the sha256 of an array, a nested result flattened to
{name: hash}, and the comparison of two such JSON files, printed as one line per group (the entry's first word, e.g.
the function called) with a digest over the group's hashes, and every entry that differs."""
import hashlib
import json


def sha(t):
    import numpy as np
    a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t))
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def flat(prefix, obj, out):
    if isinstance(obj, dict):
        out[prefix + '.keys'] = list(obj)
        for k, v in obj.items():
            flat(f'{prefix}.{k}', v, out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            flat(f'{prefix}[{i}]', v, out)
    elif hasattr(obj, 'shape'):
        out[prefix] = sha(obj)
    else:
        out[prefix] = repr(obj)


def compare(pa, pb):
    """prints the table; returns the number of entries that differ"""
    a, b = (json.load(open(p)) for p in (pa, pb))
    keys = sorted(set(a) | set(b))
    bad = [k for k in keys if a.get(k) != b.get(k)]
    print('group | entries | sha256 over the group, parent | this commit | verdict')
    for g in sorted({k.split(' ')[0] for k in keys}):
        ks = [k for k in keys if k.split(' ')[0] == g]
        da, db = (hashlib.sha256(json.dumps([d.get(k) for k in ks]).encode()).hexdigest()[:16] for d in (a, b))
        print(f"{g} | {len(ks)} | {da} | {db} | {'identical' if da == db else 'DIFFER'}")
    for k in bad:
        print(f'DIFFERS: {k}')
    print(f'{len(keys)} entries, {len(keys) - len(bad)} identical')
    return len(bad)
