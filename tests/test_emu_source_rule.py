"""The emulated source is the shipped source: under csrc/ only common.h (device primitives) and api_runtime.h (the host's view of
the HIP runtime) may part the emulator build from the product build (profiles/r21a_emu_forks.md)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "motion-diffusion-model_amd", "csrc")
MAY_TEST_MDM_EMU = {"common.h", "api_runtime.h"}
MAY_NAME_EMU_NAMESPACE = {"common.h"}
# (file, token) pairs that keep a fork of their own, each with its reason in profiles/r21a_emu_forks.md: none
EXCEPTIONS = set()


def test_emulator_forks_live_in_common_h_and_api_runtime_h():
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))
    assert len(files) > 30 and MAY_TEST_MDM_EMU <= set(files)
    bad = []
    for f in files:
        with open(os.path.join(CSRC, f)) as fh:
            text = fh.read()
        for token, allowed in ((r"\bMDM_EMU\b", MAY_TEST_MDM_EMU), (r"\bemu::", MAY_NAME_EMU_NAMESPACE)):
            n = len(re.findall(token, text))
            if n and f not in allowed and (f, token) not in EXCEPTIONS:
                bad.append(f"{f}: {n} x {token}")
    assert not bad, "emulator forks outside common.h / api_runtime.h: " + "; ".join(bad)
