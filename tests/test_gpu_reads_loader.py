"""
GPU: the device read loader (--gpu-reads) on the MI355X.  The checks of tests/test_reads_loader.py (tests/fastq_texts.py) on the HIP
engine, the 8.8 MB text whose tile sums take the scanning workgroup more than one trip, and the command lines as child processes:
`python -m badread_amd error_model | qscore_model | plot ...` with --gpu-loader --gpu-reads and without a flag.
"""
import functools
import os
import subprocess
import sys

import pytest

import fastq_texts as FT
import helpers as H

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(FT.HERE)


@functools.lru_cache(maxsize=None)
def engine():
    return H.hip_engine()


def run(command, argv):
    r = subprocess.run([sys.executable, '-m', 'badread_amd', command] + argv, cwd=REPO, capture_output=True, timeout=300)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.mark.parametrize('name', FT.FIXTURE_NAMES)
def test_texts_of_the_fixture_load_as_the_reference_loaded_them_on_the_gpu(tmp_path, name):
    FT.check_fixture_text(engine(), tmp_path, name)


def test_scan_records_of_the_committed_files_equal_the_restated_rule_on_the_gpu():
    FT.check_committed(engine())


def test_scan_records_of_the_synthetic_texts_equal_the_restated_rule_on_the_gpu():
    FT.check_synthetic(engine())


def test_scan_of_the_tile_sums_takes_more_than_one_trip_on_the_gpu():
    assert len(FT.check_scan(engine(), FT.big_text(), 0)) == 2200


def test_device_loader_equals_the_host_loader_on_the_gpu(tmp_path):
    FT.check_loader(engine(), tmp_path)


@pytest.mark.parametrize('name', sorted(FT.packed_cases()))
def test_packed_job_over_device_reads_equals_the_host_job_on_the_gpu(tmp_path, name):
    FT.check_packed_job(engine(), tmp_path, name)


def test_chunks_of_a_packed_job_do_not_show_on_the_gpu(tmp_path, monkeypatch):
    FT.check_plot_chunks(engine(), tmp_path, monkeypatch)


def test_exits_keep_their_messages_and_their_order_on_the_gpu(tmp_path, monkeypatch):
    FT.check_exits(engine(), tmp_path, monkeypatch)


def test_error_codes_of_the_abi_on_the_gpu():
    FT.check_abi(engine())


@pytest.mark.parametrize('command,extra', [('error_model', []), ('qscore_model', []), ('plot', []), ('plot', ['--qual'])])
def test_command_line_is_the_same_with_the_flags_on_the_gpu(tmp_path, command, extra):
    FT.check_cli(run, tmp_path, command, extra)


def test_flag_alone_exits_with_its_message_on_the_gpu():
    for command in ('error_model', 'qscore_model', 'plot'):
        assert 'Error: --gpu-reads needs --gpu-loader' in FT.check_flag_alone(run, command)


def test_help_lists_the_flags_on_the_gpu():
    FT.check_help(run)
