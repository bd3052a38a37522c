"""What the HIP engine refuses to run, without a GPU: ``hip_refusal`` is the
pure function behind ``HipBackend::refusal``.  Every combination of layout,
rule, boundary, census, fingerprint and ``u8_kernel=lds`` is checked against
the documented rules, written here on their own:

* a rule runs if it is compiled (B3/S23 or a line of ``life_rules.def``), and
  only B3/S23 runs on the LDS-tiled byte kernels;
* the bounded plane, the census and the fingerprint each need B3/S23 and no
  LDS-tiled byte kernels;
* the census and the fingerprint need the torus;
* the fingerprint needs an engine without the census.

A refusal names its first cause, in the order boundary, rule, census,
fingerprint, in the words the GPU tests of the engine's refusals match."""
import itertools

import pytest

DEFAULT, COMPILED, UNCOMPILED = "B3/S23", "B36/S23", "B35/S236"

CASES = list(itertools.product(("Bits", "U8"), (DEFAULT, COMPILED, UNCOMPILED), ("torus", "dead"), (False, True),
                               (False, True), (False, True)))


def _expected(layout, rule, boundary, census, fingerprint, u8_lds):
    """The phrases the refusal must start with and contain; None where the combination runs."""
    lds = layout == "U8" and u8_lds
    conway, torus = rule == DEFAULT, boundary == "torus"
    if not torus and not (conway and not lds):
        return ("boundary=dead with u8_kernel=lds" if lds else f"boundary=dead with rule {rule} on the HIP engine"), ""
    if rule == UNCOMPILED:
        return f"rule {rule}", "is not compiled for the HIP engine"
    if not conway and lds:
        return f"rule {rule}", "u8_kernel=lds"
    for on, name in ((census, "census"), (fingerprint, "fingerprint")):
        if on and not torus:
            return f"{name}=1 with boundary=dead on the HIP engine", ""
        if on and not conway:
            return f"{name}=1 with rule {rule} on the HIP engine", ""
        if on and lds:
            return f"{name}=1 with u8_kernel=lds", ""
    if fingerprint and census:
        return "fingerprint=1 with census=1 on the HIP engine", ""
    return None


def test_the_rules_of_the_cases(native):
    have = native.hip_rules()
    assert DEFAULT in have and COMPILED in have and UNCOMPILED not in have
    assert len(CASES) == 96 and len(set(CASES)) == 96


@pytest.mark.parametrize("layout,rule,boundary,census,fingerprint,u8_lds", CASES)
def test_hip_refusal(native, layout, rule, boundary, census, fingerprint, u8_lds):
    lds = layout == "U8" and u8_lds
    conway, torus = rule == DEFAULT, boundary == "torus"
    # The verdict, from the documented rules alone.
    runs = (rule != UNCOMPILED and (conway or not lds)
            and (torus or (conway and not lds))
            and (not census or (conway and not lds and torus))
            and (not fingerprint or (conway and not lds and torus and not census)))
    why = native.hip_refusal(getattr(native.Layout, layout), rule, boundary, census, fingerprint, u8_lds)
    assert (why == "") == runs, why
    want = _expected(layout, rule, boundary, census, fingerprint, u8_lds)
    assert (want is None) == runs
    if want:
        assert why.startswith(want[0]) and want[1] in why, (why, want)
