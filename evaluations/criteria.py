from linetr_amd.evaluations import descriptor_loss  # noqa: F401
