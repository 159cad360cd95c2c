"""The denoiser's surface keys (rayz_hip_denoiser_set_keys) without a GPU: the entry refuses a bad handle without
touching a device, and the exact cases the GPU test runs (denoise_keys_cases.py) are what their docstrings derive by hand."""
from fractions import Fraction as F

import numpy as np

import denoise_keys_cases as kc
from rayz_amd import capi


def test_set_keys_refuses_a_bad_handle_without_a_device(built):
    lib = capi.load()
    assert lib.rayz_hip_denoiser_set_keys(None, None) == capi.ERR_STATE and b"not a denoiser handle" in lib.rayz_hip_last_error()
    junk = (np.zeros(64, np.uint8)).ctypes.data  # (no magic: not a handle)
    assert lib.rayz_hip_denoiser_set_keys(junk, None) == capi.ERR_STATE


def test_the_exact_cases_are_their_hand_derivations():
    for case in kc.cases():
        got = case.expect()
        assert case.hand and all(got[p] == v for p, v in case.hand.items()), (case.name, {p: got[p] for p in case.hand}, case.hand)
        # .. and the rule matters in every case but the one that says a shared key changes nothing
        differs = case.expect(keyed=False) != got
        assert differs == (case.name != "one-key-two-kinds"), case.name


def test_what_the_rule_changes_in_the_first_case():
    case = kc.one_among_25()
    assert case.expect(keyed=False)[(2, 2)] == F(127, 64) and case.expect()[(2, 2)] == 1
    assert kc.background_taps().expect(keyed=False)[(0, 0)] == F(130, 11)
