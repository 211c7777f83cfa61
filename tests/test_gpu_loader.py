"""
GPU: the device loader (--gpu-loader) on the MI355X.  The checks of tests/test_loader.py (tests/paf_texts.py) on the HIP engine, the
1.1 MB text that crosses the second level of the line-start scan, and the command lines as child processes:
`python -m badread_amd error_model | qscore_model | plot ...` with and without the flag.
"""
import functools
import os
import subprocess
import sys

import pytest

import helpers as H
import paf_texts as PT

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(PT.HERE)


@functools.lru_cache(maxsize=None)
def engine():
    return H.hip_engine()


def run(command, argv):
    r = subprocess.run([sys.executable, '-m', 'badread_amd', command] + argv, cwd=REPO, capture_output=True, timeout=300)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_scan_records_of_the_committed_files_equal_the_host_parse_on_the_gpu():
    PT.check_committed(engine())


@pytest.mark.parametrize('name', ['edges_files', 'mixed'])
def test_scan_records_of_the_made_files_equal_the_host_parse_on_the_gpu(name):
    PT.check_made_files(engine(), name)


def test_scan_records_of_the_synthetic_text_equal_the_host_parse_on_the_gpu():
    PT.check_synthetic(engine())


def test_scan_crosses_the_second_level_of_the_line_start_scan_on_the_gpu():
    assert len(PT.check_scan(engine(), PT.big_text(), irregular=0)) == 18000


@pytest.mark.parametrize('name', PT.ODD_NAMES)
def test_irregular_lines_are_flagged_and_parsed_like_the_reference_on_the_gpu(tmp_path, name):
    PT.check_odd_line(engine(), tmp_path, name)


def test_carriage_returns_and_high_bytes_take_the_host_loader_on_the_gpu(tmp_path):
    PT.check_host_route(engine(), tmp_path)


def test_device_loader_equals_the_host_loader_on_the_gpu(tmp_path):
    PT.check_selection(engine(), tmp_path)


@pytest.mark.parametrize('name', sorted(PT.packed_cases()))
def test_packed_job_equals_the_host_job_on_the_gpu(tmp_path, name):
    PT.check_packed_job(engine(), tmp_path, name)


def test_chunks_of_a_packed_job_do_not_show_on_the_gpu(tmp_path, monkeypatch):
    PT.check_plot_chunks(engine(), tmp_path, monkeypatch)


def test_exits_keep_their_messages_and_their_order_on_the_gpu(tmp_path):
    PT.check_exits(engine(), tmp_path)


def test_error_codes_of_the_abi_on_the_gpu():
    PT.check_abi(engine())


@pytest.mark.parametrize('command,extra', [('error_model', []), ('qscore_model', []), ('plot', []), ('plot', ['--qual']),
                                           ('plot', ['--qual', '--max_alignments', '7'])])
def test_command_line_is_the_same_with_the_flag_on_the_gpu(tmp_path, command, extra):
    PT.check_cli(run, tmp_path, command, extra)


def test_help_lists_the_flag_on_the_gpu():
    PT.check_help(run)
