"""CPU: the command line of the streamed path (`python -m fcvsr_amd.sr`) parses without a GPU."""
import pytest

from fcvsr_amd import sr
from fcvsr_amd.harness import surfaces


def test_help_and_the_option_list(capsys):
    with pytest.raises(SystemExit) as e:
        sr.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--model", "--weights", "--size", "--pix-fmt", "--out-pix-fmt", "--batch", "--ensemble", "--tile", "--cuts",
                "--output-size", "SRC", "DST"):
        assert opt in text
    assert sr.PIX_FMTS == surfaces.PIX_FMTS


def test_arguments():
    a = sr.parser().parse_args(["--model", "FCVSR_SNet", "--weights", "w.pth", "--size", "480x270", "--pix-fmt", "p010le", "--cuts",
                                "auto", "--output-size", "1440x810", "--tile", "128x64", "-", "-"])
    assert a.size == (480, 270) and a.pix_fmt == "p010le" and a.out_pix_fmt is None and a.cuts == "auto"
    assert a.output_size == (1440, 810) and a.tile == (128, 64) and a.src == "-" and a.dst == "-" and a.batch == 8
    assert sr.parser().parse_args(["--model", "GShiftNet", "--weights", "w", "--size", "8x8", "--cuts", "5,9", "a", "b"]).cuts == [5, 9]
    for bad in (["--size", "480"], ["--size", "axb"], ["--pix-fmt", "yuv422p"], ["--model", "EDVR"]):
        with pytest.raises(SystemExit):
            sr.parser().parse_args(["--model", "GShiftNet_S", "--weights", "w", "--size", "8x8", "a", "b"] + bad)
