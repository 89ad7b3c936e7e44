"""The five ctypes bindings over canu_amd/_capi.py, with no GPU: each module's error class, its
loader, and the atoi / atof that find_errors re-exports."""
import pytest

from canu_amd import _capi
from canu_amd import correct_overlaps, falconsense, find_errors, pair, trim_reads

BINDINGS = [(find_errors, "FeError", "FE_STATUS"), (correct_overlaps, "CoError", "CO_STATUS"),
            (pair, "PairError", "PAIR_STATUS"), (falconsense, "FsError", "FS_STATUS"),
            (trim_reads, "TrError", "TR_STATUS")]
IDS = [m.__name__.rsplit(".", 1)[1] for m, _, _ in BINDINGS]


@pytest.mark.parametrize("mod,err,status", BINDINGS, ids=IDS)
def test_error_class_names_the_status(mod, err, status):
    E, names = getattr(mod, err), getattr(mod, status)
    assert sorted(names) == list(range(-7, 1))
    for code, name in names.items():
        e = E(code, "a message")
        assert isinstance(e, RuntimeError) and e.code == code
        assert str(e) == f"{name}: a message"
        assert name.startswith(status[:-len("STATUS")])
    assert str(E(-99, "m")) == "-99: m" and E(-99, "m").code == -99


@pytest.mark.parametrize("mod,err,status", BINDINGS, ids=IDS)
def test_load_library_is_cached(built, mod, err, status):
    lib = mod.load_library()
    assert lib is mod.load_library()
    for name in mod.EXPORTS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("mod,err,status", BINDINGS, ids=IDS)
def test_missing_library_raises_the_modules_error(monkeypatch, tmp_path, mod, err, status):
    monkeypatch.setattr(mod, "_lib", None)
    gone = str(tmp_path / "no_such_library.so")
    with pytest.raises(getattr(mod, err)) as ei:
        mod.load_library(gone)
    assert ei.value.code == -1 and gone in str(ei.value)
    assert str(ei.value).startswith(getattr(mod, status)[-1] + ": ")
    assert mod._lib is None


def test_atoi_atof_are_still_find_errors():
    for s, i, f in (("", 0, 0.0), (" +12x", 12, 12.0), ("-3", -3, -3.0), (".5e1", 0, 5.0),
                    ("1e", 1, 1.0), ("abc", 0, 0.0)):
        assert find_errors._atoi(s) == _capi._atoi(s) == i, s
        assert find_errors._atof(s) == _capi._atof(s) == f, s
