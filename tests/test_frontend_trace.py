"""The front-end's launch decisions (spec.hip: spec_route; cqt.hip: basis_route, the pyramid chain, scale_launch; cqt_dec.hip: dec_route)
against the trace recorded before they became one route per file.  CPU only: tests/san/frontend_trace.cpp is a stand-alone program built
from the sanitizer objects of tests/san/build_san.py and the recording shim, so AddressSanitizer and UBSan are part of the executable."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'san'))


def test_front_end_launches_are_those_of_the_recorded_trace():
    """tests/golden/frontend_trace.json was recorded by tests/san/frontend_trace.py on commit e996752, BEFORE spec_power_launch, cqt.hip's
    launchers and amtx_launch_cqt_decimate took their decisions from spec_route, basis_route / scale_launch / the one pyramid chain and
    dec_route.  Once per front-end switch (none, AMTX_SPEC_NO_RING, AMTX_CQT_COPY_LEVEL0, AMTX_CQT_GEMM_BASIS, AMTX_CQT_DECIM_V1,
    AMTX_CQT_DECIM_BLOCKS=64), each in a child process of its own: the return code, error text and every launch (kernel name with its template
    arguments, grid, block, dynamic LDS bytes) of
      - amtx_spec_power and amtx_spec_power_clips for ten plans (ring; general with mel weights in LDS at 64 and 68 tap slots, from memory at
        104, without mel stage; pow2 with mel and at n_fft 128 and 4096; not centred; reflecting pad -- the tap slots are
        amtx_spec_mel_layout's, recorded too) at six (batch, samples) each, the last refused ("grid too large");
      - every CQT entry point (forward, forward16, forward16_split, track_layout, pyramid_build, power_clips, clips, clips16, clips16_split,
        the two workspace queries, num_frames, and both scaled forms with a workspace 256 bytes short) for the plans of cqt_ref.PLANS at each
        librosa version they list, CQT 84 / 12 over cqt_ref.SWEEP, HCQT 6 x 72, nine harmonics and a plan mixing n_fft 256 and 128, at batch
        1, 3 and 512 (pyramid_build at 512 tracks for the two flagship plans only).
    Every row has to come back; a report of either sanitizer fails the child."""
    import build_san
    import frontend_trace
    if not os.path.exists(build_san.HIPCC):
        pytest.skip('no hipcc: the sanitizer build needs the ROCm clang')
    got = frontend_trace.record()
    with open(os.path.join(ROOT, 'tests', 'golden', 'frontend_trace.json')) as f:
        golden = json.load(f)
    cases = frontend_trace.cases()
    assert golden['cases_sha256'] == frontend_trace.cases_sha256() and len(cases) == 1793       # the golden rows are in the order of this list
    want = frontend_trace.expand(golden)
    assert tuple(want) == frontend_trace.SWITCHES == tuple(got)
    for switch in frontend_trace.SWITCHES:
        g, w = got[switch], want[switch]
        assert len(g) == len(w) == len(cases)
        wrong = [(c, a, b) for c, a, b in zip(cases, g, w) if a != b]
        assert not wrong, (switch, 'rows (case, got, want)', len(wrong), wrong[:5])
