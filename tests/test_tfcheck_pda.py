"""The module side of K14: ``validation_pda_check`` puts ``NTM_PDA_CHECK=1`` into the Job's
environment and nothing else changes; the README tables are current."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
STACK_DIR = ROOT / "modules" / "amd-gpu-stack"


def _stack_local(name, **overrides):
    from nvidia_terraform_modules_amd.tfcheck.config import load_module
    from nvidia_terraform_modules_amd.tfcheck.evaluate import Evaluator, Scope, convert

    mod = load_module(STACK_DIR)
    ev = Evaluator()
    variables = {}
    for vn, v in mod.variables.items():
        if vn in overrides:
            variables[vn] = overrides[vn]
        elif not v.required:
            variables[vn] = convert(ev.eval(v.block.body.attr("default"), Scope({}, {})), v.type_expr)
    scope = Scope(variables, {n: e for n, (e, _, _) in mod.locals.items()}, str(mod.path))
    return ev.eval(mod.locals[name][0], scope)


def test_module_sets_the_variable_only_when_asked():
    off, on = _stack_local("validation_env"), _stack_local("validation_env", validation_pda_check=True)
    assert "NTM_PDA_CHECK" not in off and on["NTM_PDA_CHECK"] == "1"
    assert {k: v for k, v in on.items() if k != "NTM_PDA_CHECK"} == off
    args = _stack_local("validation_args")
    assert _stack_local("validation_args", validation_pda_check=True) == args
    assert not [a for a in args if "pda" in a]
    text = (STACK_DIR / "variables.tf").read_text()
    block = text.split('variable "validation_pda_check"')[1].split("\n}")[0]
    assert "bool" in block and "false" in block and "profiles/pda/README.md" in block


def test_readme_tables_are_current():
    p = subprocess.run([sys.executable, "-m", "nvidia_terraform_modules_amd.tfcheck", "--docs-check", str(STACK_DIR)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0 and "0 README(s) stale" in p.stdout, p.stdout + p.stderr
    assert "validation_pda_check" in (STACK_DIR / "README.md").read_text()
