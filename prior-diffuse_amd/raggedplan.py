"""Host-side planner of the batched file loop (``ComplexDDPMTrainer.generate_wav(batch=N)``): which files are decoded
together, in which order their noise is drawn, and which of them share a padded batch.  Pure functions of counts and lengths -
no device, no files - so that the order of everything that touches the random generator can be checked on its own.

The loop takes the sorted path list in WINDOWS of ``8 * batch`` consecutive paths.  Inside a window every readable file's x_T is
drawn in path order (so file k's noise does not depend on ``batch``); the files are then sorted by length, cut into BUCKETS of
``batch`` and each bucket is enhanced as one exact ragged batch whose padded length is rounded up to a multiple of ``QUANTUM``
samples, so that geometries recur in the plan cache.  Results are written in path order.
"""
WINDOW_BATCHES = 8      # a window holds this many buckets: enough files for the length sort to keep the padding small
QUANTUM = 2560          # padded lengths are multiples of 16 frames (160 ms)


def windows(n_paths, batch):
    """[(first, last + 1)] of the windows over ``n_paths`` sorted paths."""
    if batch < 1:
        raise ValueError("batch must be at least 1")
    step = WINDOW_BATCHES * int(batch)
    return [(i, min(i + step, n_paths)) for i in range(0, int(n_paths), step)]


def padded_length(n, quantum=QUANTUM):
    return -(-int(n) // quantum) * quantum


def buckets(lens, batch, quantum=QUANTUM):
    """lens: the lengths (samples) of a window's readable files, in path order.  Returns [(indices, L_pad)]: indices into
    ``lens``, every one exactly once; files sorted by (length, position) - equal lengths keep path order, so the result is a
    function of the lengths alone - and cut into runs of ``batch``; L_pad: the longest of the run rounded up to ``quantum``."""
    if batch < 1:
        raise ValueError("batch must be at least 1")
    order = sorted(range(len(lens)), key=lambda i: (int(lens[i]), i))
    out = []
    for j in range(0, len(order), int(batch)):
        idx = order[j:j + int(batch)]
        out.append((idx, padded_length(max(int(lens[i]) for i in idx), quantum)))
    return out


def padding_waste(lens, batch, quantum=QUANTUM):
    """Padded frames / own frames of ``buckets(lens, batch)`` (1.0: no padding)."""
    own = sum(1 + int(n) // 160 for n in lens)
    padded = sum(len(idx) * (1 + L_pad // 160) for idx, L_pad in buckets(lens, batch, quantum))
    return padded / max(own, 1)
