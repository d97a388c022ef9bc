"""The generator's build-time knobs (csrc/gen_kernels.py, no GPU needed): every ``EELG_*`` name
it reads from the environment is a row of its one knob table, and a retired knob set to a value
other than the shipped one stops ``main`` before anything is written -- a variant build must not
compile the default under the variant's label."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "energy-equiv-lattice-gnn_amd", "csrc")
if CSRC not in sys.path:
    sys.path.insert(0, CSRC)

import gen_kernels as gk  # noqa: E402

SOURCE = open(os.path.join(CSRC, "gen_kernels.py")).read()
# an environment read of a literal name: _knob("X"), os.environ.get("X"), os.environ["X"], os.getenv("X")
READ = re.compile(r"""(?:_knob|environ\.get|environ|getenv)\s*[\(\[]\s*["'](EELG_\w+)["']""")


def test_every_environment_read_is_a_row_of_the_knob_table():
    read = set(READ.findall(SOURCE))
    assert read == set(gk.KNOBS)
    # one helper does the reading: no other mention of the environment besides the retired check
    assert SOURCE.count("os.environ") == 2
    for name, default in gk.KNOBS.items():
        assert isinstance(default, int) and name.startswith("EELG_")
        if name not in os.environ:
            assert getattr(gk, name[len("EELG_"):]) == default


def test_no_retired_name_is_read():
    assert not set(gk.RETIRED_KNOBS) & set(gk.KNOBS)
    for name in gk.RETIRED_KNOBS:
        # its one mention is its row of the retired table; no module variable is left of it
        assert len(re.findall(rf"\b{name}\b", SOURCE)) == 1, name
        assert not hasattr(gk, name[len("EELG_"):]), name


@pytest.mark.parametrize("name", sorted(gk.RETIRED_KNOBS))
def test_retired_knob_at_another_value_stops_main_before_it_writes(name, monkeypatch, tmp_path, capsys):
    shipped = gk.RETIRED_KNOBS[name]
    monkeypatch.setenv(name, "dual" if isinstance(shipped, str) else str(shipped + 1))
    with pytest.raises(SystemExit) as exc:
        gk.main(tmp_path)
    assert exc.value.code not in (0, None)
    assert name in str(exc.value.code) + capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("name", sorted(gk.RETIRED_KNOBS))
def test_retired_knob_at_its_shipped_value_is_accepted(name, monkeypatch):
    monkeypatch.setenv(name, str(gk.RETIRED_KNOBS[name]))
    gk.check_retired_knobs()


def test_other_eelg_names_are_ignored(monkeypatch):
    for name in gk.RETIRED_KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("EELG_OVERLAP", "0")
    monkeypatch.setenv("EELG_LIB", "/nowhere/libeelg.so")
    gk.check_retired_knobs()
    gk.check_retired_knobs({"EELG_OVERLAP": "0", "EELG_TP_BWF": "1"})
