"""Workload models: the validation Job (flagship) and the cluster
time-to-GPU-ready phase model."""
from .validation_job import (GemmWorkload, ValidationConfig, ValidationReport,  # noqa: F401
                             cu_sweep_check, hbm_memtest, host_link_check, mx_check,
                             run_validation, xcd_sweep_check, atomics_check, mcore_check, mxq_check,
                             wave_check)
