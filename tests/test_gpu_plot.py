"""
GPU: `badread plot` on the MI355X.  The checks of tests/test_plot.py (tests/plot_windows.py) on the HIP engine, and the command line
as a child process: `python -m badread_amd plot ...` with the real engine.
"""
import functools
import io
import os
import subprocess
import sys

import pytest

import helpers as H
import plot_windows as PW
from badread_amd import __main__ as cli
from badread_amd import plot_window_identity as P

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(PW.HERE)


@functools.lru_cache(maxsize=None)
def engine():
    return H.hip_engine()


def run(argv):
    r = subprocess.run([sys.executable, '-m', 'badread_amd', 'plot'] + argv, cwd=REPO, capture_output=True, timeout=300)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_window_means_equal_the_reference_on_the_gpu():
    PW.check_fixture(engine())


@pytest.mark.parametrize('name', sorted(PW.synthetic_jobs()))
def test_window_means_equal_the_restatement_on_the_gpu(name):
    job3, windows = PW.synthetic_jobs()[name]
    PW.check_against_restatement(engine(), job3, windows)


def test_error_codes_of_the_abi_on_the_gpu(monkeypatch):
    PW.check_abi(engine(), monkeypatch)


def test_chunks_do_not_show_on_the_gpu(monkeypatch):
    PW.check_chunking(engine(), monkeypatch)


@pytest.mark.parametrize('window,qual', PW.CLI_CASES)
def test_command_line_on_the_gpu(tmp_path, monkeypatch, window, qual):
    def chunked(argv):                          # a child process cannot lower the constant: the same call in this process
        out = io.StringIO()
        with monkeypatch.context() as m:
            m.setattr(P, 'PLOT_CHUNK_BASES', 3000)
            P.plot_window_identity(cli.parse_args(['plot'] + argv), output=out, engine=engine(), stdout=out)
        return 0, out.getvalue(), ''
    PW.check_cli(run, tmp_path, chunked, [(window, qual)])


def test_command_line_errors_on_the_gpu(tmp_path):
    PW.check_cli_errors(run, tmp_path)


def test_save_writes_one_png_per_alignment_on_the_gpu(tmp_path):
    pytest.importorskip('matplotlib')
    PW.check_cli_save(run, tmp_path)
