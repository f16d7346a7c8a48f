"""Shared by tools/make_golden_frozen.py (writes the frozen-BatchNorm fixtures) and the tests that read them.

A summarize_grads() dict of the full model (520 tensors, up to 2 048 fp32 samples each) compresses to about 1.9 MB, above
the 1 MiB limit for a committed file, so the gradient fixtures are stored in parts: `<name>.npz` holds the names, the norms
and the first tensors' samples, `<name>_part2.npz`, ... the remaining samples.  load_grads() returns the merged dict, in
the form golden_util.compare_grads / grad_rel_errors expect."""
import os

import numpy as np

import golden_util as G

MAX_FILE_BYTES = 1 << 20
PART_BUDGET = 1_000_000          # uncompressed sample bytes per part (fp32 mantissas barely compress: ~0.93 of their size)


def _part_path(name, i):
    return os.path.join(G.GOLDEN_DIR, name + (".npz" if i == 1 else "_part%d.npz" % i))


def save_grads(name, d):
    """Write a summarize_grads() dict as `<name>.npz` + `<name>_part<i>.npz`, each below the committed-file limit."""
    os.makedirs(G.GOLDEN_DIR, exist_ok=True)
    parts, cur, used = [], {"names": d["names"], "norms": d["norms"]}, 0
    for n in d["names"]:
        a = np.ascontiguousarray(d["g:" + str(n)])
        if used + a.nbytes > PART_BUDGET and used:
            parts.append(cur)
            cur, used = {}, 0
        cur["g:" + str(n)] = a
        used += a.nbytes
    parts.append(cur)
    paths = []
    for i, p in enumerate(parts, 1):
        path = _part_path(name, i)
        np.savez_compressed(path, **p)
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, "%s: %d bytes" % (path, size)
        print("wrote %s (%.1f KB)" % (path, size / 1024))
        paths.append(path)
    if os.path.exists(_part_path(name, len(parts) + 1)):       # a stale part of an earlier, longer split
        raise RuntimeError("remove the stale %s first" % _part_path(name, len(parts) + 1))
    return paths


def load_grads(name):
    d = dict(np.load(_part_path(name, 1)))
    i = 2
    while os.path.exists(_part_path(name, i)):
        d.update(np.load(_part_path(name, i)))
        i += 1
    missing = [str(n) for n in d["names"] if "g:" + str(n) not in d]
    assert not missing, "%s: no samples for %s" % (name, missing[:3])
    return d


BUFFER_SUFFIXES = (".running_mean", ".running_var", ".num_batches_tracked")


def buffers_of(state_dict):
    """{name: clone} of every BatchNorm buffer of a state dict."""
    return {k: v.detach().clone() for k, v in state_dict.items() if k.endswith(BUFFER_SUFFIXES)}
