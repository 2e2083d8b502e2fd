"""The reference's ``util`` package: the canvas helpers of the joint box -> layout -> image edit (``data_util``), the script
reader and the tensor -> picture converters (``util``), the result page (``html``) and the ``Visualizer``."""
