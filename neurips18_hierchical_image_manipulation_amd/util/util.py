"""``load_script_to_opt`` (reference util/util.py:46-63): the options a shell script would pass, parsed by an options
class."""
import re


def load_script_to_opt(script_path, opt_class):
    """A one-line script passes everything after ``python <driver>.py``; a multi-line script (one ``--flag value \\`` per
    line) passes the lines whose first word is a flag the options class knows, minus the line's last word (the trailing
    backslash).  Quotes are dropped.  Same rules as upstream, indented lines and a final line without a backslash
    included."""
    dummy_opt = opt_class().parse(save=False, default_args=[])
    with open(script_path, 'r') as f:
        lines = f.readlines()
    if len(lines) == 1:
        options = [option.strip('\n') for option in lines[0].split(' ')[2:]]
    else:
        options = []
        for line in lines:
            option = re.sub('["\']', '', line).split(' ')
            if hasattr(dummy_opt, option[0].strip('--')):
                options += option[:-1]
    return opt_class().parse(save=False, default_args=options)
