#!/usr/bin/env python3
"""Record oracle/_ref's answers to what tests/test_oracle_vs_ref.py asks it, into tests/golden/ref_answers.npz.

Run where the reference checkout is (oracle/Makefile's REF), after a change to what those tests ask the reference:
    python tests/golden/make_ref_answers.py
The tests run once against the built oracle/_ref through a recorder (oracle_lib.RefAnswers); where oracle/_ref cannot be
built, the `ref` fixture answers the same calls from the file.  The file holds data only: a hash of each call's arguments
and the bytes, bins, states and statuses the reference returned.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib  # noqa: E402
import test_oracle_vs_ref as t  # noqa: E402


def main():
    ref = oracle_lib.load_ref()
    assert ref is not None, "needs the reference checkout to build oracle/_ref"
    oracle = oracle_lib.load_oracle()
    answers = oracle_lib.RefAnswers()
    rec = answers.recorder(ref)
    t.test_half_coder_matches_reference(oracle, rec)
    for adaptive in (False, True):                       # the parametrisation of test_recoded_coder_matches_reference
        t.test_recoded_coder_matches_reference(oracle, rec, adaptive)
    t.test_recoded_zero_probability_is_reported(oracle, rec)
    t.test_cabac_instantiation_matches_reference_coder(oracle, rec)
    answers.save(oracle_lib.REF_ANSWERS)
    print(oracle_lib.REF_ANSWERS, len(answers.table), "answers,", os.path.getsize(oracle_lib.REF_ANSWERS), "bytes")


if __name__ == "__main__":
    main()
