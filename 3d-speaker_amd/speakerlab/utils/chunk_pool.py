"""Batch plan for embedding the sub-segments of several files together (``--pool_chunks``).

Host-only bookkeeping.  The reference pads every sub-segment of a file to that file's longest
one (``do_emb_extraction``'s ``max_len``), so a file's chunks keep their own pad length here;
chunks of different files can share a batch only when their files pad alike.
"""
from collections import namedtuple

import numpy as np

# one batch of the plan: its pad length and, row by row, the (file, chunk) it embeds
ChunkBatch = namedtuple('ChunkBatch', ['pad_len', 'files', 'chunks'])


def plan_chunk_batches(lens_per_file, batchsize):
    """``lens_per_file[f]``: the chunk lengths (samples) of file ``f``, possibly none.

    Returns ``(batches, inverse)``.  ``batches`` is a list of ``ChunkBatch``: chunks are grouped by
    their file's pad length (the maximum chunk length of the file), groups come in the order of
    their first file, (file, chunk) order is kept inside a group, and every group is cut into
    batches of at most ``batchsize`` rows.  ``inverse[f]`` is an int64 array with the row of every
    chunk of file ``f`` in the concatenation of the batches' outputs, so ``rows[inverse[f]]`` is
    file ``f``'s embeddings in chunk order (an empty array for a file without chunks).
    """
    batchsize = int(batchsize)
    if batchsize < 1:
        raise ValueError('plan_chunk_batches: batchsize must be at least 1')
    groups = {}                      # pad length -> [(file, chunk), ...] (dicts keep insertion order)
    for f, lens in enumerate(lens_per_file):
        lens = np.asarray(lens, dtype=np.int64).reshape(-1)
        if lens.size == 0:
            continue
        if int(lens.min()) < 1:
            raise ValueError(f'plan_chunk_batches: file {f} has an empty chunk')
        groups.setdefault(int(lens.max()), []).extend((f, c) for c in range(lens.size))
    batches = []
    inverse = [np.empty(len(np.asarray(lens).reshape(-1)), dtype=np.int64) for lens in lens_per_file]
    row = 0
    for pad_len, members in groups.items():
        for lo in range(0, len(members), batchsize):
            part = np.asarray(members[lo:lo + batchsize], dtype=np.int64)
            batches.append(ChunkBatch(pad_len, part[:, 0].copy(), part[:, 1].copy()))
            for f, c in part:
                inverse[f][c] = row
                row += 1
    return batches, inverse
