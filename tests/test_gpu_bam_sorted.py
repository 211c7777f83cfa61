"""
GPU: --truth-bam-sorted on the MI355X.  The emulated-device checks of tests/test_bam_sorted.py on the HIP engine (sort and gather, the
BGZF grid, the index and the two ABIs against the plain-Python restatement of tests/bam_sorted.py, the records of simulated batches), the
command line (both files independent of streams and batch sizes, FASTQ and --truth-bam unchanged by the option, tags and formats in the
records) and two ranks on one GPU.
"""
import os

import pytest

import bam_sorted as BS
import helpers as H
import test_gpu_truth_paf as GP
import test_truth_bam as TB
import test_truth_sam as TS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', BS.sort_cases(), ids=lambda c: c[0])
def test_sort_and_gather_equal_the_stable_sort_on_the_gpu(case):
    BS.check_sort_case(H.hip_engine(), case)


@pytest.mark.parametrize('case', BS.grid_cases(), ids=lambda c: c[0])
def test_the_blocks_and_their_offsets_on_the_gpu(case):
    BS.check_grid_case(H.hip_engine(), case)


@pytest.mark.parametrize('case', BS.index_cases(), ids=lambda c: c[0])
def test_the_index_equals_the_restatement_on_the_gpu(case):
    BS.check_index_case(H.hip_engine(), case)


def test_brx_bam_sort_abi_on_the_gpu():
    BS.check_sort_abi(H.hip_engine())


def test_brx_bam_index_abi_on_the_gpu():
    BS.check_index_abi(H.hip_engine())


def test_the_records_of_simulated_batches_sorted_on_the_gpu():
    BS.check_batches(H.hip_engine, 400, 512, 1)


def _pair(tmp_path, name):
    return (tmp_path / name).read_bytes(), (tmp_path / (name + '.bai')).read_bytes()


def test_truth_bam_sorted_from_the_cli(tmp_path):
    pref, _ = TS.small()
    bam = lambda name: ['--truth-bam', str(tmp_path / name)]
    ordered = lambda name: ['--truth-bam-sorted', str(tmp_path / name)]
    plain, _ = GP.run_cli(tmp_path, None, *bam('plain.bam'))
    fq, _ = GP.run_cli(tmp_path, None, *bam('a.bam'), *ordered('a.sorted.bam'))
    assert fq == plain and (tmp_path / 'a.bam').read_bytes() == (tmp_path / 'plain.bam').read_bytes()
    _, records = TB.split_bam((tmp_path / 'plain.bam').read_bytes(), pref)
    blob, bai = _pair(tmp_path, 'a.sorted.bam')
    f = BS.check_file_pair(blob, bai, pref, records)
    assert len(f.recs) > 100
    for i, extra in enumerate((['--gpu-streams', '1', '--gpu-batch', '64'], ['--gpu-streams', '3', '--gpu-batch', '200'])):      # the option alone
        fq, _ = GP.run_cli(tmp_path, None, *extra, *ordered(f'b{i}.bam'))
        assert fq == plain and _pair(tmp_path, f'b{i}.bam') == (blob, bai), extra
    # tags and formats go into the records of this file as into --truth-bam's
    extra = ['--truth-tags', 'MD,SA', '--truth-cs', 'short', '--truth-eqx']
    fq, _ = GP.run_cli(tmp_path, None, *extra, *bam('t.bam'), *ordered('t.sorted.bam'))
    assert fq == plain
    _, tagged = TB.split_bam((tmp_path / 't.bam').read_bytes(), pref)
    assert tagged != records
    BS.check_file_pair(*_pair(tmp_path, 't.sorted.bam'), pref, tagged)


def test_truth_bam_sorted_of_two_ranks_on_one_gpu(tmp_path):
    import collections
    import test_gpu_cli as C
    pref, _ = TS.small()
    single_fq, _ = GP.run_cli(tmp_path, None, '--truth-bam-sorted', str(tmp_path / 'single.bam'), quantity='40x')
    single = _pair(tmp_path, 'single.bam')
    whole = BS.check_file_pair(*single, pref)
    path = tmp_path / 'ranks.bam'
    out = C._launch_ranks(tmp_path, 2, ['--truth-bam-sorted', str(path)], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'))
    assert open(out, 'rb').read() == single_fq and _pair(tmp_path, 'ranks.bam') == single
    prefix, spath = str(tmp_path / 'shard'), str(tmp_path / 'shard.bam')
    C._launch_ranks(tmp_path, 2, ['--output-shards', prefix, '--truth-bam-sorted', spath], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'),
                    out_name='unused.fastq')
    parts = [BS.check_file_pair(*_pair(tmp_path, f'shard.bam.{r}'), pref) for r in range(2)]
    count = lambda files: collections.Counter(r['raw'] for f in files for r in f.recs)
    assert all(len(f.recs) > 0 for f in parts) and count(parts) == count([whole])
    assert not os.path.exists(spath) and not os.path.exists(spath + '.bai')
