"""Shared by test_gpu_ba.py, test_gpu_sim3.py, test_gpu_sim3_opt.py and test_gpu_pnp.py: the schedule that wraps a solver's ring of
problem tables and crosses its workspace between streams.  2 x ring + 1 calls of the device form, enqueued on two alternating side streams
with no synchronisation between them; problem counts rise and fall, so a slot of the ring is reused by a larger call (regrown) and by a
smaller one; one call past the middle is larger than every call before it (the workspace grows behind a host wait), smaller ones follow
(they wait on the stream).  When other tests of the process ran the solver first, the workspace is already large and every call takes
the stream wait; run alone, a test file starts with this test."""
RING = 8              # SD_SOLVER_RING (csrc/sd_api.hip)
COUNTS = [1, 3, 2, 6, 1, 4, 2, 5, 3, 1, 8, 2, 1, 4, 2, 3, 2]
BIG = 10


def schedule(pool, size):
    """The problems of each call: call BIG takes the COUNTS[BIG] largest of `pool` (by size(problem) > 0: correspondences or edges), the
    others walk round the rest."""
    assert len(COUNTS) == 2 * RING + 1 and max(COUNTS) <= 8 and COUNTS[BIG] == max(COUNTS) and BIG > len(COUNTS) // 2
    assert any(COUNTS[k + RING] > COUNTS[k] for k in range(RING)) and any(COUNTS[k + RING] < COUNTS[k] for k in range(RING))
    order = sorted(pool, key=size)
    big, rest = order[-COUNTS[BIG]:], order[:-COUNTS[BIG]]
    assert len(rest) >= max(COUNTS) and size(rest[-1]) > 0
    calls, at = [], 0
    for k, n in enumerate(COUNTS):
        calls.append(big if k == BIG else [rest[(at + j) % len(rest)] for j in range(n)])
        at += 0 if k == BIG else n
    totals = [sum(size(p) for p in c) for c in calls]
    assert totals[BIG] > max(totals[:BIG]) and totals[BIG] > max(totals[BIG + 1:])
    return calls


def drive(calls, prepare, enqueue):
    """prepare(problems) -> the torch-owned arrays of one call (all made before the first call); enqueue(arrays, stream handle) calls the
    device form.  Returns the arrays of every call after ONE synchronisation of the two streams."""
    import torch
    prepared = [prepare(c) for c in calls]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()                                  # the uploads above; nothing below waits until the end
    for k, a in enumerate(prepared):
        enqueue(a, streams[k % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    return prepared
