"""The reference's ``util`` helpers that the joint box -> layout -> image edit needs (util/data_util.py, util/util.py
upstream); the visualiser and the HTML writer are not built."""
