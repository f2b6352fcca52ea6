"""Drop-in mirror of the reference staticstics/ package (its spelling): the feature frames from the transaction log
(preprosess_agg_parallel) and the customer personas clustered from it (preprocess_clustering)."""
