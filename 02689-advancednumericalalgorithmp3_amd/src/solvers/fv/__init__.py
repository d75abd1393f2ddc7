"""Finite-volume SIMPLE solver of the lid-driven cavity (the reference's ``solver: fv``), advanced by the HIP kernel
of include/ldc_fv.h.  Importing needs no GPU; constructing a solver does."""
