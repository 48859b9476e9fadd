"""Host side of clips cut from resident tracks (amt_tools_amd/tracks.py): the descriptor table amtx_spec_power_clips reads is built and
validated by a pure function, the first frame follows the reference's rule, and the new entry point reports errors.  No GPU here."""
import pickle

import numpy as np
import pytest

from amt_tools_amd import _lib
from amt_tools_amd.tracks import TrackBank, clip_descriptors, frame_start

# a bank of three tracks at hop 512, centred: 1 + n // 512 frames each
LENGTHS = np.array([40000, 5000, 1500])
STARTS = np.array([0, 40000, 45000])
FRAMES = 1 + LENGTHS // 512            # 79, 10, 3


def test_descriptor_table_of_valid_requests():
    desc = clip_descriptors(STARTS, LENGTHS, FRAMES, [0, 0, 0, 1, 2], [0, 37, 79 - 3, 7, 0], 3)
    assert desc.dtype == np.int64 and desc.shape == (5, 4) and desc.flags['C_CONTIGUOUS']
    np.testing.assert_array_equal(desc, [[0, 40000, 0, 3], [0, 40000, 37, 3], [0, 40000, 76, 3], [40000, 5000, 7, 3], [45000, 1500, 0, 3]])
    # a clip may be a whole track, and a reflect-padded plan is fine with tracks longer than n_fft / 2
    np.testing.assert_array_equal(clip_descriptors(STARTS, LENGTHS, FRAMES, [1], [0], 10, reflect_half=1024), [[40000, 5000, 0, 10]])
    np.testing.assert_array_equal(clip_descriptors(STARTS, LENGTHS, FRAMES, np.array([2]), np.array([1]), 2, reflect_half=1024), [[45000, 1500, 1, 2]])


@pytest.mark.parametrize('track_ids,first_frames,num_frames,reflect_half,match', [
    ([3], [0], 1, None, 'unknown track 3'),
    ([-1], [0], 1, None, 'unknown track -1'),
    ([0], [-1], 4, None, 'negative first frame'),
    ([0], [77], 3, None, 'run past the 79 frames of track 0'),        # one frame too far
    ([0, 1], [0, 8], 3, None, 'clip 1: .* run past the 10 frames'),
    ([2], [0], 4, None, 'run past the 3 frames of track 2'),          # a track shorter than the clip
    ([0, 2], [0, 0], 2, 2048, 'track 2 has 1500 samples: reflect padding'),
    ([0], [0], 0, None, 'at least one frame'),
    ([0, 1], [0], 2, None, 'one first frame per track id'),
])
def test_invalid_requests_raise(track_ids, first_frames, num_frames, reflect_half, match):
    with pytest.raises(ValueError, match=match):
        clip_descriptors(STARTS, LENGTHS, FRAMES, track_ids, first_frames, num_frames, reflect_half=reflect_half)


def test_reflect_bound_is_n_fft_half_exactly():
    """amtx_spec_power's own rule: reflect padding needs MORE than n_fft / 2 samples."""
    args = ([0], [1025], [3], [0], [0], 1)
    clip_descriptors(*args, reflect_half=1024)
    with pytest.raises(ValueError, match='reflect padding'):
        clip_descriptors([0], [1024], [3], [0], [0], 1, reflect_half=1024)
    clip_descriptors([0], [1024], [3], [0], [0], 1, reflect_half=None)


def test_frame_start_is_the_reference_rule():
    """amt_tools/datasets/common.py:392: frame_start = sample_start // hop_length, hand-written values."""
    for sample_start, hop, want in ((0, 512, 0), (511, 512, 0), (512, 512, 1), (513, 512, 1), (2559, 512, 4), (2560, 512, 5),
                                    (44100, 512, 86), (319999, 512, 624), (1000, 128, 7), (np.int64(16000 * 30), 512, 937)):
        assert frame_start(sample_start, hop) == want and isinstance(frame_start(sample_start, hop), int)


def test_bank_bookkeeping_needs_no_gpu_and_pickles_without_device_state():
    from amt_tools_amd.features import CQT, MelSpec
    rng = np.random.default_rng(0)
    tracks = [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]
    bank = TrackBank(tracks, MelSpec(sample_rate=16000, hop_length=512))
    np.testing.assert_array_equal(bank.starts, STARTS)
    np.testing.assert_array_equal(bank.lengths, LENGTHS)
    np.testing.assert_array_equal(bank.frame_counts, FRAMES)
    assert len(bank) == 3 and '_dev' not in bank.__dict__                  # nothing touched a device
    again = pickle.loads(pickle.dumps(bank))
    np.testing.assert_array_equal(again._host, np.concatenate(tracks))
    np.testing.assert_array_equal(again.frame_counts, FRAMES)
    bank.__dict__['_dev'] = ('audio', 'db_ref')                            # stands for the device tensors
    assert '_dev' not in pickle.loads(pickle.dumps(bank)).__dict__
    with pytest.raises(NotImplementedError, match='no clip form'):
        TrackBank(tracks, CQT())
    with pytest.raises(NotImplementedError, match='no clip form'):
        CQT().process_clips(None)
    with pytest.raises(ValueError, match='reflect padding'):
        TrackBank(tracks[:2] + [tracks[2][:1024]], MelSpec(sample_rate=16000, librosa_version='0.9'))
    with pytest.raises(ValueError, match='non-empty 1-D'):
        TrackBank([np.zeros((2, 100), dtype=np.float32)], MelSpec())


def test_entry_point_reports_a_null_plan():
    with pytest.raises(_lib.AmtxError, match='amtx_spec_power_clips.*null argument'):
        _lib.call('amtx_spec_power_clips', None, None, None, 1, 1, None, None, None)
    with pytest.raises(TypeError, match='amtx_spec_power_clips takes 8'):
        _lib.call('amtx_spec_power_clips', None, None, None, 1, 1, None, None)


def test_power_kernels_keep_their_registers_and_do_not_spill():
    """The ring and general power kernels are launch-bounded to 2 waves per SIMD (256 VGPRs) and live near that bound; a spill to scratch
    in the frame loop would cost more than anything the kernels do.  spec.hip, device code only, with the build's own flags: the
    equal-clips instantiations keep the parent's VGPR counts (ring 250; general 227 / 235 / 215; power-of-two 38), every
    instantiation has no scratch, and the clips forms of the ring and general kernels stay at 2 waves per SIMD."""
    import os
    import re
    import subprocess
    from amt_tools_amd import build
    src = os.path.join(build.CSRC, 'spec.hip')
    cmd = [build.HIPCC] + build.FLAGS + build.FILE_FLAGS['spec.hip'] + ['-x', 'hip', '--cuda-device-only', '-c', src, '-o', os.devnull,
                                                                        '-Rpass-analysis=kernel-resource-usage']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    for block in re.split(r'remark: Function Name: ', r.stderr)[1:]:
        name = block.split()[0]
        if 'spec_power' in name:
            found[name] = tuple(int(re.search(pat + r': (\d+)', block).group(1)) for pat in (r' VGPRs', r'ScratchSize \[bytes/lane\]', r'Occupancy \[waves/SIMD\]'))
    print(found)

    def one(*parts):
        hits = [v for k, v in found.items() if all(part in k for part in parts)]
        assert len(hits) == 1, (parts, sorted(found))
        return hits[0]
    parent = {('ring_kernel',): 250, ('spec_power_kernelILi8ELb1ELb1E',): 227, ('spec_power_kernelILi8ELb1ELb0E',): 235,
              ('spec_power_kernelILi8ELb0ELb0E',): 215, ('pow2_kernel',): 38}
    assert len(found) == 10
    for parts, vgprs in parent.items():
        assert one(*parts, 'EqualClips') == (vgprs, 0, 8 if parts == ('pow2_kernel',) else 2), parts
        v, scratch, waves = one(*parts, 'ClipTable')
        assert scratch == 0 and waves >= (8 if parts == ('pow2_kernel',) else 2) and v <= 256, (parts, v, scratch, waves)
