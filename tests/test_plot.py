"""
`badread plot` (badread_amd/plot_window_identity.py, brx_window_means, csrc/brx_window.h) without a GPU: the plain-Python restatement of
the window identities against the fixture recorded from the running reference, and the product -- the kernels interpreted on the CPU
(tests/emu_engine.py) under the host code -- against the fixture and against the restatement.  The checks are those of
tests/plot_windows.py; tests/test_gpu_plot.py runs the same on the MI355X.
"""
import functools
import io

import pytest

import emu_engine as EE
import plot_windows as PW
from badread_amd import __main__ as cli
from badread_amd import plot_window_identity as P


@functools.lru_cache(maxsize=None)
def emu():
    return EE.EmuEngine(scratch_bytes=1 << 20)


def run(argv):
    """`plot` with the interpreted engine: (exit status, stdout, message)"""
    out = io.StringIO()
    try:
        P.plot_window_identity(cli.parse_args(['plot'] + argv), output=out, engine=emu(), stdout=out)
    except SystemExit as e:
        return 1, out.getvalue(), str(e.code)
    return 0, out.getvalue(), ''


def test_restatement_equals_the_reference():
    PW.check_restatement_against_fixture()


def test_window_means_equal_the_reference():
    PW.check_fixture(emu())


@pytest.mark.parametrize('name', sorted(PW.synthetic_jobs()))
def test_window_means_equal_the_restatement(name):
    job3, windows = PW.synthetic_jobs()[name]
    PW.check_against_restatement(emu(), job3, windows)


def test_error_codes_of_the_abi(monkeypatch):
    PW.check_abi(emu(), monkeypatch)


def test_chunks_do_not_show(monkeypatch):
    PW.check_chunking(emu(), monkeypatch)


def test_trailing_deletion_is_refused_on_the_host():
    PW.check_trailing_deletion()


@pytest.mark.parametrize('window,qual', PW.CLI_CASES)
def test_command_line(tmp_path, monkeypatch, window, qual):
    def chunked(argv):
        with monkeypatch.context() as m:
            m.setattr(P, 'PLOT_CHUNK_BASES', 3000)
            return run(argv)
    PW.check_cli(run, tmp_path, chunked, [(window, qual)])


def test_command_line_errors(tmp_path):
    PW.check_cli_errors(run, tmp_path)


def test_matplotlib_is_needed_for_drawing_only(monkeypatch):
    import sys
    for name in [m for m in sys.modules if m == 'matplotlib' or m.startswith('matplotlib.')]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, 'matplotlib', None)             # importing it now raises ImportError
    status, out, _ = run(PW.FILE_ARGS + ['--no_plot', '--max_alignments', '4'])
    assert status == 0 and out.count('\n') == 6
    for draw in ([], ['--no_plot', '--save', 'plots']):
        status, out, message = run(PW.FILE_ARGS + ['--max_alignments', '4'] + draw)
        assert status == 1 and message == 'Error: plot needs matplotlib to display or save plots (use --no_plot)'


def test_save_writes_one_png_per_alignment(tmp_path):
    pytest.importorskip('matplotlib')
    PW.check_cli_save(run, tmp_path)
