"""Drop-in mirror of the reference utils/monitor package (the ranker's training rows)."""
