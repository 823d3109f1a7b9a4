"""avr_test_hook_set (the -DAVR_TEST_HOOKS build of the library) knows the hooks of TestHooks and no others.  No call here touches a device."""
import pytest


def test_retired_k1_form_hooks_are_unknown_hooks(avr):
    """The hooks that chose the one-lane-per-slice K1's measured coder forms left the library with those forms, and the two tuning
    switches no test set (chain_lanes, k1_waves) after them: the setter answers their names like any name it does not know; a hook
    that stayed is accepted."""
    for name in ("k1_form_ref", "k1_emit_lds", "k1_fwd", "k1_words8", "chain_lanes", "k1_waves"):
        with pytest.raises(avr.AvrError, match=f"unknown test hook {name}$"):
            with avr.test_hooks(**{name: 1}):
                pass
    with avr.test_hooks(census_stride=16) as handle:
        assert handle is avr.lib()
