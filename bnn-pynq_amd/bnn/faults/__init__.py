"""Fault-injection campaigns (mirror of the reference's ``bnn.faults``, bnn/faults/faults.py)."""
from .faults import HARDENING_SCHEMES, CNVFaultTest, FaultTest, LFCFaultTest, NetworkTest, hardening_of  # noqa: F401

__version__ = "0.1"
