"""Host side of utterances in flight (no device needed): the argument errors of ``enhance_stream`` and ``generate_wav(inflight=)``,
the argument errors of the operator's new mode (csrc/range.hip: PDSE_RANGE_NONFINITE), and what ``SamplerPipeline(verdict=)`` records."""
import re
import os

import pytest

from conftest import ROOT, pkg


def _bare_trainer(**attrs):
    """A trainer object without a device: only what the argument checks read."""
    T = pkg("trainer").ComplexDDPMTrainer
    tr = object.__new__(T)
    tr.audit = False
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


@pytest.mark.parametrize("bad", [0, 5, -1, 17])
def test_inflight_outside_1_to_4_is_refused(bad):
    tr = _bare_trainer()
    with pytest.raises(ValueError, match="inflight"):
        tr.enhance_stream([], inflight=bad)                      # at the call, not at the first next()
    with pytest.raises(ValueError, match="inflight"):
        tr.generate_wav(inflight=bad)


def test_batches_and_the_audit_do_not_stream():
    tr = _bare_trainer()
    with pytest.raises(ValueError, match="batch"):
        tr.generate_wav(batch=2, inflight=2)
    with pytest.raises(ValueError, match="batch"):
        tr.generate_wav(batch=8, inflight=4)
    with pytest.raises(ValueError, match="audit"):
        _bare_trainer(audit=True).enhance_stream([], inflight=3)


def test_cli_flag():
    src = open(os.path.join(ROOT, "prior-diffuse_amd", "main.py")).read()
    assert re.search(r'"--inflight", type=int, default=1', src) and "inflight=args.inflight" in src


def test_argument_errors_of_the_nonfinite_mode_need_no_device():
    L = pkg("_lib")
    L.load()
    hdr = open(os.path.join(ROOT, "include", "pdse.h")).read()
    assert re.search(r"#define PDSE_RANGE_NONFINITE (\d+)", hdr).group(1) == str(L.RANGE_NONFINITE) == "2"
    d = L.RangeDesc()
    d.mode, d.out_rows, d.nrows, d.blocks = L.RANGE_NONFINITE, 2, 1, 1
    d.rows, d.out = 4096, None                                    # never followed: the descriptor is refused first
    with pytest.raises(L.PdseError, match="null"):
        L.launch(d)
    d.rows, d.out = None, 4096
    with pytest.raises(L.PdseError, match="null row table"):
        L.launch(d)
    d.rows, d.nrows = 4096, 3
    with pytest.raises(L.PdseError, match="more rows than the output table"):
        L.launch(d)
    d.nrows = 0
    with pytest.raises(L.PdseError, match="zero rows"):
        L.launch(d)
    d.nrows, d.blocks = 1, 0
    with pytest.raises(L.PdseError, match="blocks"):
        L.launch(d)


def test_verdict_false_is_the_plan_as_it_was_and_true_adds_two_launches(weights):
    L = pkg("_lib")
    P = pkg("pipeline").SamplerPipeline
    args = ("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 1)
    kinds = lambda p: [type(d) for d, _ in p.descs]   # noqa: E731
    plain = P(*args, L_=1600)
    off = P(*args, L_=1600, verdict=False)
    assert kinds(off) == kinds(plain) and list(off.ranges.items()) == list(plain.ranges.items())
    assert not off.verdict and off.verdict_tab is None and not any(isinstance(d, L.RangeDesc) for d, _ in off.descs)
    with pytest.raises(ValueError, match="verdict"):
        off.verdict_fetch()
    with pytest.raises(ValueError, match="verdict"):
        off.verdict_counts()

    on = P(*args, L_=1600, verdict=True)
    assert len(on.descs) == len(plain.descs) + 2
    first, last = on.descs[0][0], on.descs[-1][0]
    assert isinstance(first, L.RangeDesc) and isinstance(last, L.RangeDesc)
    assert kinds(on)[1:-1] == kinds(plain) and L.KIND_OF[type(first)] == L.KIND_OF[type(last)] == L.OP_RANGE
    assert first.mode == L.RANGE_CLEAR and last.mode == L.RANGE_NONFINITE
    assert first.out == last.out == on.verdict_tab.data_ptr() and first.out_rows == last.out_rows == last.nrows == 2
    assert tuple(on.verdict_tab.shape) == (2, L.RANGE_BINS)
    assert on.ranges["verdict"] == (len(on.descs) - 1, len(on.descs)) and on.ranges["stft"][0] == 0
    # without the signal back end only the spectrogram is judged
    spec_only = P(*args, T=11, verdict=True)
    assert spec_only.descs[-1][0].nrows == 1 and tuple(spec_only.verdict_tab.shape) == (1, L.RANGE_BINS)
    assert len(spec_only.descs) == len(P(*args, T=11).descs) + 2
    with pytest.raises(ValueError, match="verdict"):
        pkg("planfile").save_pipeline("unused.plan", on)
    with pytest.raises(L.PdseError, match="CPU context"):
        on.verdict_fetch()
