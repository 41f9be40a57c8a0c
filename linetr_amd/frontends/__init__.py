"""Upstream producers of the LineTR hot path that this package supplies itself.  linetr_amd.matching looks here for a module the host
project's models/ does not hold: line_detector.LSD (the native line segment detector)."""
