"""create_auditor: the closed-loop certificate auditor behind the plugin surface (new: the
reference has no counterpart; built like create_evaluator)."""
from ..trainer.certificate_auditor import CertificateAuditor
from ..trainer.robustness_auditor import RobustnessAuditor
from .registry import Registry

registry = Registry("auditor")
registry.register("certificate_auditor", CertificateAuditor)
# the same auditor plus sweep(): the closed loop under sensor / actuator noise levels
registry.register("robustness_auditor", RobustnessAuditor)


def create_auditor(auditor_name: str = "certificate_auditor", **kwargs):
    au = registry.build(auditor_name, **kwargs)
    print(auditor_name, "created successfully!")
    return au
