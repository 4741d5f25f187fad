"""nlps_host_read_materials on the Newtonian-Fluid-Compressible block (InOutFun/Material/Fluid/Compressible-Newtonian-Fluid.c:
60-175): the accepted block, every missing-parameter refusal of :155-199, the Fbar refusal, and keys the reader does not know."""
import importlib

import pytest

from util import nlps

gid = importlib.import_module("nl-partsol_amd.gid")

WATER = """Define-Material(idx=0,Model=Newtonian-Fluid-Compressible)
{
  rho=1000
  Compressibility=2.2e9
  Reference-Pressure=101325
  Viscosity=1.0e-3
  Macdonald-parameter=7.15
}
Define-Material(idx=1,Model=Neo-Hookean-Wriggers)
{
  rho=2000
  E=1.0e7
  nu=0.3
}
"""
KEYS = ("rho", "Compressibility", "Reference-Pressure", "Viscosity", "Macdonald-parameter")


def _line(key):
    return next(l + "\n" for l in WATER.split("\n") if l.strip().startswith(key + "="))


def test_the_fluid_block_is_read(tmp_path):
    p = tmp_path / "run.nlp"
    p.write_text(WATER)
    (i0, rho0, m0), (i1, rho1, m1) = gid.read_materials(p)
    assert (i0, rho0, m0["type"]) == (0, 1000.0, 6) and (i1, rho1, m1["type"]) == (1, 2000.0, 0)
    assert (m0["compressibility"], m0["p_ref"], m0["viscosity"], m0["n_macdonald"]) == (2.2e9, 101325.0, 1.0e-3, 7.15)
    assert (m0["E"], m0["nu"]) == (0.0, 0.0)
    assert (m1["viscosity"], m1["compressibility"], m1["n_macdonald"]) == (0.0, 0.0, 0.0)
    # F-bar switched off is the reference's default and is read over, its alpha with it
    p.write_text(WATER.replace("  rho=1000\n", "  rho=1000\n  Fbar=false\n  Fbar-alpha=0.5\n"))
    assert gid.read_materials(p)[0][2]["viscosity"] == 1.0e-3


@pytest.mark.parametrize("key", KEYS)
def test_every_missing_parameter_is_refused(tmp_path, key):
    p = tmp_path / "run.nlp"
    p.write_text(WATER.replace(_line(key), "", 1))
    with pytest.raises(nlps().NlpsError, match="Some parameter is missed for Compressible Newtonian Fluid material: " + key):
        gid.read_materials(p)


def test_fbar_and_unknown_keys_are_refused(tmp_path):
    E = nlps().NlpsError
    p = tmp_path / "run.nlp"
    p.write_text(WATER.replace("  rho=1000\n", "  rho=1000\n  Fbar=true\n"))
    with pytest.raises(E, match="Fbar needs"):
        gid.read_materials(p)
    for extra, msg in (("  E=1.0e7\n", "Undefined E"), ("  nu=0.3\n", "Undefined nu"), ("  Ceps=1.5\n", "Undefined Ceps"),
                       ("  Reference-pressure=1.0\n", "Undefined Reference-pressure")):
        p.write_text(WATER.replace("  rho=1000\n", "  rho=1000\n" + extra, 1))
        with pytest.raises(E, match=msg):
            gid.read_materials(p)
    p.write_text(WATER.replace("Newtonian-Fluid-Compressible", "Newtonian-Fluid-Incompressible"))
    with pytest.raises(E, match="not one of the laws"):
        gid.read_materials(p)
