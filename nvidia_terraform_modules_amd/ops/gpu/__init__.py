"""Device wrappers of the opt-in checks (K4 to K12), one module per check; import the module you need."""
