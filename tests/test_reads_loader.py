"""
The device read loader (--gpu-reads: brx_fastq_scan, brx_reads_pack, csrc/brx_fastqin.h; reads.load_fastq_device, model_builder.Job.packed
over a DeviceReads) without a GPU: the kernels interpreted on the CPU (tests/emu_engine.py) under the host code, against the fixture
recorded from the running reference, a restatement of its state machine and the host's own loader and packer.  The checks are those of
tests/fastq_texts.py; tests/test_gpu_reads_loader.py runs the same on the MI355X.
"""
import functools
import io

import pytest

import emu_engine as EE
import fastq_texts as FT
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
        if isinstance(e.code, str):
            err.write(e.code + '\n')
        return (1 if isinstance(e.code, str) else e.code or 0), out.getvalue(), err.getvalue()
    return 0, out.getvalue(), err.getvalue()


@pytest.mark.parametrize('name', FT.FIXTURE_NAMES)
def test_texts_of_the_fixture_load_as_the_reference_loaded_them(tmp_path, name):
    FT.check_fixture_text(emu(), tmp_path, name)


def test_scan_records_of_the_committed_files_equal_the_restated_rule():
    FT.check_committed(emu())


def test_scan_records_of_the_synthetic_texts_equal_the_restated_rule():
    FT.check_synthetic(emu())


def test_device_loader_equals_the_host_loader(tmp_path):
    FT.check_loader(emu(), tmp_path)


@pytest.mark.parametrize('name', sorted(FT.packed_cases()))
def test_packed_job_over_device_reads_equals_the_host_job(tmp_path, name):
    FT.check_packed_job(emu(), tmp_path, name)


def test_chunks_of_a_packed_job_do_not_show(tmp_path, monkeypatch):
    FT.check_plot_chunks(emu(), tmp_path, monkeypatch)


def test_exits_keep_their_messages_and_their_order(tmp_path, monkeypatch):
    FT.check_exits(emu(), tmp_path, monkeypatch)


def test_error_codes_of_the_abi():
    FT.check_abi(emu())


@pytest.mark.parametrize('command,extra', [('error_model', ['--max_alignments', '12']), ('qscore_model', ['--max_alignments', '12']),
                                           ('plot', []), ('plot', ['--qual'])])
def test_command_line_is_the_same_with_the_flags(tmp_path, command, extra):
    FT.check_cli(run, tmp_path, command, extra)


@pytest.mark.parametrize('command', ['error_model', 'qscore_model', 'plot'])
def test_flag_alone_exits_with_its_message(command):
    assert 'Error: --gpu-reads needs --gpu-loader' in FT.check_flag_alone(run, command)


def test_help_lists_the_flags(capsys):
    def helped(command, argv):
        with pytest.raises(SystemExit) as e:
            cli.parse_args([command] + argv)
        return e.value.code, capsys.readouterr().out, ''
    FT.check_help(helped)
