"""The window schedule of a long recording: pure functions on integers, no device and no torch.

A recording of T frames is enhanced with ONE plan of W frames.  What grows with T and is small stays whole-file (waveforms,
[B,2,T,161] spectrograms, the frame GEMMs of the front and back end); the two networks run on windows [a, a + W) of the
whole-file tensors.  A network with a finite receptive field (H_left frames back, H_right ahead: ``receptive_field()`` of the plan
builders in nets.py) gives, on a window, exactly the whole-file values for every frame that lies at least H_left behind the
window's start and H_right before its end - or at the start / end of the file itself, where the window's zero padding IS the
network's.  ``windows`` cuts [0, T) into such kept ranges.  A network whose past is a recurrent state (``carries_state``: the GCRN
prior) runs on consecutive windows instead, the state handed on: ``carried``.
"""

FRAME_TILE = 32           # frames per tile of the kernels that tile the frames (csrc/tcm2.hip, the chunks of csrc/lstm.hip)
# --window given without a value: 2048 frames, 20.5 s of signal - a multiple of FRAME_TILE, 2.7 times the 766 frames of the
# eps-net's two halos (388 + 378), so 1282 of every 2048 frames computed are kept
DEFAULT_WINDOW = 2048


def window_arg(window):
    """``window`` of the entry points: None (off), or an int that is a positive multiple of FRAME_TILE; anything else: ValueError."""
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int) or window < FRAME_TILE or window % FRAME_TILE:
        raise ValueError("window must be a positive multiple of %d frames (the kernels' frame tile), got %r" % (FRAME_TILE, window))
    return window


def round_up(frames):
    """The smallest multiple of FRAME_TILE that is >= frames."""
    return -(-int(frames) // FRAME_TILE) * FRAME_TILE


def windows(T, W, H_left, H_right):
    """[(a, keep_lo, keep_hi)]: windows [a, a + W) of a T-frame file and the frames [keep_lo, keep_hi) each one owns.

    0 <= a <= T - W; the first window starts at 0 and the last ends at T, so the file's own edges see the network's own zero
    padding and no halo is invented there; every kept frame lies at least H_left behind its window's start and H_right before
    its end unless that edge is the file's; the kept ranges partition [0, T) in order.  The last window is clamped to T - W and
    overlaps its neighbour by more than the halos.  T <= W: the single whole-file window (0, 0, T).  W <= H_left + H_right (no
    frame of a middle window could be kept): ValueError."""
    T, W, H_left, H_right = int(T), int(W), int(H_left), int(H_right)
    if T < 1 or W < 1 or H_left < 0 or H_right < 0:
        raise ValueError("windows: T >= 1, W >= 1 and halos >= 0, got T=%d W=%d H=(%d, %d)" % (T, W, H_left, H_right))
    if W <= H_left + H_right:
        raise ValueError("window of %d frames does not exceed the receptive field, %d + %d frames: no frame of a window inside the "
                         "file would see all of its inputs" % (W, H_left, H_right))
    if T <= W:
        return [(0, 0, T)]
    out, lo = [], 0
    while True:
        a = max(0, lo - H_left) if lo else 0
        if a + W >= T:
            out.append((T - W, lo, T))
            return out
        hi = a + W - H_right
        out.append((a, lo, hi))
        lo = hi


def carried(T, W):
    """[(a, keep_lo, keep_hi)] for a network that carries its state: consecutive windows [k W, (k + 1) W) in time order, each
    owning all of its frames.  The last one may hang over the end of the file (a + W > T): the network is causal, so what the
    frames behind T hold reaches no frame before T, and they are not kept."""
    T, W = int(T), int(W)
    if T < 1 or W < 1:
        raise ValueError("carried: T >= 1 and W >= 1, got T=%d W=%d" % (T, W))
    return [(a, a, min(a + W, T)) for a in range(0, T, W)]


def recompute_ratio(W, H_left, H_right):
    """Frames computed per frame kept by a window inside the file: W / (W - H_left - H_right), the price of exactness."""
    return W / float(W - H_left - H_right)


def window_conflicts(**flags):
    """The options a windowed pass cannot be combined with, as one ValueError naming the first that is set.  flags: ragged,
    members, inflight, per_channel, objective, plan_file, verdict, label, graph - whatever the caller has."""
    why = {
        "ragged": "exact ragged batches mask whole-file kernels by every utterance's own length",
        "members": "a posterior ensemble runs K trajectories through one whole-file plan",
        "inflight": "utterances in flight share the GPU between whole-file plans, a windowed pass runs its windows one after the other",
        "per_channel": "per-channel enhancement batches a file's channels through one whole-file plan",
        "objective": "the objective plan is one eps-net step of a padded batch",
        "plan_file": "a plan file holds one recorded plan; a windowed pass is a loop around two",
        "verdict": "the in-flight verdict judges one recorded plan",
        "label": "the label leg belongs to the validation pass of a whole-file plan",
        "graph": "a windowed pass is a host loop around a window plan, not one recorded plan",
    }
    for name, value in flags.items():
        on = value > 1 if name in ("members", "inflight") and not isinstance(value, bool) else bool(value)
        if on:
            raise ValueError("window= with %s: %s (windowed passes enhance one padded batch, one trajectory, one file at a time)"
                             % (name if isinstance(value, bool) or name not in ("members", "inflight") else "%s=%d" % (name, value),
                                why[name]))
