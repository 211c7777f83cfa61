"""
The device loader (--gpu-loader: brx_paf_scan, brx_align_pack, csrc/brx_pafin.h; alignment.load_alignments_device, model_builder.Job.packed)
without a GPU: the kernels interpreted on the CPU (tests/emu_engine.py) under the host code, against the host's own loader and packer and
against the fixture recorded from the running reference.  The checks are those of tests/paf_texts.py; tests/test_gpu_loader.py runs the
same on the MI355X.
"""
import functools
import io

import pytest

import emu_engine as EE
import paf_texts as PT
from badread_amd import __main__ as cli
from badread_amd import model_builder as MB
from badread_amd import plot_window_identity as P


@functools.lru_cache(maxsize=None)
def emu():
    return EE.EmuEngine(scratch_bytes=1 << 26)


def run(command, argv):
    """A command with the interpreted engine: (exit status, stdout, the text on `output`)"""
    out, err = io.StringIO(), io.StringIO()
    try:
        args = cli.parse_args([command] + argv)
        if command == 'plot':
            P.plot_window_identity(args, output=out, engine=emu(), stdout=out)
        else:
            (MB.make_error_model if command == 'error_model' else MB.make_qscore_model)(args, output=err, engine=emu(), stdout=out)
    except SystemExit as e:
        return (1 if isinstance(e.code, str) else e.code or 0), out.getvalue(), err.getvalue()
    return 0, out.getvalue(), err.getvalue()


def test_scan_records_of_the_committed_files_equal_the_host_parse():
    PT.check_committed(emu())


@pytest.mark.parametrize('name', ['edges_files', 'mixed'])
def test_scan_records_of_the_made_files_equal_the_host_parse(name):
    PT.check_made_files(emu(), name)


def test_scan_records_of_the_synthetic_text_equal_the_host_parse():
    PT.check_synthetic(emu())


@pytest.mark.parametrize('name', PT.ODD_NAMES)
def test_irregular_lines_are_flagged_and_parsed_like_the_reference(tmp_path, name):
    PT.check_odd_line(emu(), tmp_path, name)


def test_carriage_returns_and_high_bytes_take_the_host_loader(tmp_path):
    PT.check_host_route(emu(), tmp_path)


def test_device_loader_equals_the_host_loader(tmp_path):
    PT.check_selection(emu(), tmp_path)


@pytest.mark.parametrize('name', sorted(PT.packed_cases()))
def test_packed_job_equals_the_host_job(tmp_path, name):
    PT.check_packed_job(emu(), tmp_path, name)


def test_chunks_of_a_packed_job_do_not_show(tmp_path, monkeypatch):
    PT.check_plot_chunks(emu(), tmp_path, monkeypatch)


def test_exits_keep_their_messages_and_their_order(tmp_path):
    PT.check_exits(emu(), tmp_path)


def test_error_codes_of_the_abi():
    PT.check_abi(emu())


@pytest.mark.parametrize('command,extra', [('error_model', ['--max_alignments', '12']), ('qscore_model', ['--max_alignments', '12']),
                                           ('plot', []), ('plot', ['--qual']), ('plot', ['--qual', '--max_alignments', '7'])])
def test_command_line_is_the_same_with_the_flag(tmp_path, command, extra):
    PT.check_cli(run, tmp_path, command, extra)


def test_help_lists_the_flag(capsys):
    def helped(command, argv):
        with pytest.raises(SystemExit) as e:
            cli.parse_args([command] + argv)
        return e.value.code, capsys.readouterr().out, ''
    PT.check_help(helped)
