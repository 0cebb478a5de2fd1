"""CPU oracle of the MFSR hot path -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this package, and only as the checker.  Pinned to the reference (where it has a kernel): see oracle_common.h.
"""
