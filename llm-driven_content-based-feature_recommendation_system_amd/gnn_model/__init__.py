"""Drop-in mirrors of the reference gnn_model/ modules (LightGCL, the distillation of its scores)."""
