"""Drop-in mirror of the reference staticstics/ package (its spelling): the feature frames from the transaction log."""
