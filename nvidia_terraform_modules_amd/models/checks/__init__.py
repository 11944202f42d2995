"""The opt-in checks of the validation Job (K4 to K12) as Python models, one module per check."""
