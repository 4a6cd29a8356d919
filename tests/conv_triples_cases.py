"""The three-role case of convolution-shaped triples: tests/three_role_cases.py's "batch" case under
ProtocolForm(conv_triples=True), registered by name where tests/party_worker.py looks cases up.  Run as a program it IS that
worker (`out case pf seed`), with the case known to it.  A module of helpers, not of tests."""
import os
import runpy
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.three_role_cases import CASES, Case  # noqa: E402


class ConvTriplesCase(Case):
    def form(self):
        import dataclasses

        return dataclasses.replace(super().form(), conv_triples=True)


CASES["conv-triples"] = ConvTriplesCase(*CASES["batch"])

if __name__ == "__main__":
    runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "party_worker.py"), run_name="__main__")
